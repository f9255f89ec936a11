"""-m gpu: the openings on the domain for a batch of polynomials in one pass (kzg_all.hip: plk_kzg_open_all_batch_dev) and the batched G1
transform underneath (g1ntt.hip: plk_g1_ntt_batch_dev) — every stage launch covers all the transforms, the polynomial is the slow index.

Referees.  The G1 batch: plk_g1_ntt_dev of every row.  The proofs: plk_kzg_open_all_dev per polynomial; the trapdoor of the tau = 42 key,
pi_i = ((f(42) - f(omega^i)) / (42 - omega^i)) G by ol.ntt, ol.vbatch_inv and ol.g1_mul, at (5, 3) and after a change of the key; the verdicts
of plk_kzg_verify_many_dev.  Affine coordinates are unique: every comparison is an equality of bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD
from tests.gen import fk20_cases as fk

ERR_ARG, ERR_SIZE, ERR_SRS = 1, 2, 3
TAU = 42
TOP = 0x30644e72e131a029                                        # top limb of r: four limbs with a smaller top one are a residue
G = ol.g1_generator()
INF = np.zeros(8, dtype=np.uint64)
AA = 0xAAAAAAAAAAAAAAAA
CANARY = 5                                                      # rows of 0xAA behind entry count * N of every output
# about 0: the kept transform costs an empty event pair (0.005 ms measured); building it is log_n + 2 launches, each stage of
# which is a whole scalar multiplication (0.85 ms).  The bound sits a factor 4 below one stage and a factor 40 above the empty pair.
KEPT_MS = 0.2


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key_points(ctx):
    """2048 points tau^j G of the tau = 42 key, computed once by the device: inputs of the G1 batch (no CPU scalar multiplication)"""
    ctx.srs_generate(2048, 0, TAU)
    pts = ctx.srs_download(0, 2048)
    pts.setflags(write=False)
    return pts


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _host(t, width):
    return t.cpu().numpy().view(np.uint64).reshape(-1, width)


def _rand_fr(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, size=n, dtype=np.uint64)
    return a


def _g(k):
    return ol.g1_mul(G, k % R_MOD) if k % R_MOD else INF.copy()


def _points(logs):
    return np.stack([_g(k) for k in logs])


def _trapdoor_proofs(coeffs, log_n, tau):
    """every pi_i from the secret: ((f(omega^i) - f(tau)) / (omega^i - tau)) G; also the values f(omega^i)"""
    n = 1 << log_n
    vals = ol.ntt(coeffs, log_n)
    num = ol.vadd_scalar(vals, -ol.poly_eval(coeffs, tau))
    den = ol.vbatch_inv(ol.vadd_scalar(ol.vpowers(ol.omega(log_n), n), -tau))
    return _points(ol.fr_ints(ol.vmul(num, den))), vals


def _mixed(count, log_n, seed=3):
    """count polynomials back to back, the kinds of fk20_cases.POLY_KINDS in turn (the zero and constant rows give identity and zero lanes
    beside full ones), a fresh seed per row"""
    return np.concatenate([ol.fr_vec(fk.poly(fk.POLY_KINDS[(b + 4) % len(fk.POLY_KINDS)], log_n, seed + b)) for b in range(count)])


def _open_batch(ctx, d_polys, count, log_n, values=False, evals=True):
    """-> (proofs, evals) of the batch call; the canary rows behind count * N of both outputs are checked here"""
    total = count << log_n
    d_proofs = _dev(np.full((total + CANARY, 8), AA, dtype=np.uint64))
    d_evals = _dev(np.full((total + CANARY, 4), AA, dtype=np.uint64)) if evals else None
    ctx.kzg_open_all_batch_dev(d_polys, count, log_n, d_proofs, evals_ptr=d_evals, values=values)
    proofs = _host(d_proofs, 8)
    assert (proofs[total:] == AA).all(), (log_n, count)
    if not evals:
        return proofs[:total], None
    ev = _host(d_evals, 4)
    assert (ev[total:] == AA).all(), (log_n, count)
    return proofs[:total], ev[:total]


def _open_single(ctx, d_poly, log_n, values=False):
    n = 1 << log_n
    d_proofs, d_evals = _dev(np.full((n, 8), AA, dtype=np.uint64)), _dev(np.full((n, 4), AA, dtype=np.uint64))
    ctx.kzg_open_all_dev(d_poly, log_n, d_proofs, evals_ptr=d_evals, values=values)
    return _host(d_proofs, 8), _host(d_evals, 4)


def _singles(ctx, polys, count, log_n, values=False):
    n = 1 << log_n
    rows = [_open_single(ctx, _dev(polys[b * n:(b + 1) * n]), log_n, values=values) for b in range(count)]
    return np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])


# ------------------------------------------------------------------------------------------------ the G1 batch against the single transform
# (2, 37): 74 butterflies, many transforms in one wave and a ragged tail; (7, 5): 320, a transform straddles two workgroups and the last
# workgroup is partial; (8, 3): the re-indexing seam of g1ntt_stage
@pytest.mark.parametrize("log_n,count", [(1, 1), (2, 37), (5, 3), (6, 5), (7, 5), (8, 3), (9, 3)])
def test_g1_batch_is_the_single_transform_of_every_row(ctx, key_points, log_n, count):
    n, total = 1 << log_n, count << log_n
    rng = np.random.default_rng(900 + log_n)
    start = int(rng.integers(0, 2048 - total + 1))
    pts = key_points[start:start + total].copy()
    pts[rng.choice(total, size=(total + 4) // 5, replace=False)] = 0                      # identities among the points
    if (log_n, count) == (9, 3):
        pts[n:2 * n] = 0                                                                  # one row is all identities
    d_in = _dev(pts)
    for inverse in (False, True):
        want = np.empty_like(pts)
        d_one = _dev(np.zeros((n, 8), dtype=np.uint64))
        for b in range(count):
            ctx.g1_ntt_dev(_dev(pts[b * n:(b + 1) * n]), log_n, d_one, inverse=inverse)
            ctx.synchronize()
            want[b * n:(b + 1) * n] = _host(d_one, 8)
        d_out = _dev(np.full((total + CANARY, 8), AA, dtype=np.uint64))
        ctx.g1_ntt_batch_dev(d_in, count, log_n, d_out, inverse=inverse)                  # out of place
        ctx.synchronize()
        out = _host(d_out, 8)
        assert np.array_equal(out[:total], want), (log_n, count, inverse)
        assert (out[total:] == AA).all(), (log_n, count, inverse)
        assert np.array_equal(_host(d_in, 8), pts), (log_n, count, inverse)
        d_place = _dev(pts)
        ctx.g1_ntt_batch_dev(d_place, count, log_n, d_place, inverse=inverse)             # in place
        ctx.synchronize()
        assert np.array_equal(_host(d_place, 8), want), (log_n, count, inverse)
        ctx.g1_ntt_batch_dev(d_place, count, log_n, d_place, inverse=not inverse)         # the round trip returns the input bytes
        ctx.synchronize()
        assert np.array_equal(_host(d_place, 8), pts), (log_n, count, inverse)
        if (log_n, count) == (9, 3):
            assert not want[n:2 * n].any()


# ------------------------------------------------------------------------------------------------ the proofs against the single call
@pytest.mark.parametrize("log_n,count", [(0, 3), (1, 5), (2, 37), (3, 3), (4, 17), (6, 5), (7, 3), (8, 2), (10, 2), (5, 1)])
def test_every_row_is_plk_kzg_open_all_devs(ctx, log_n, count):
    n = 1 << log_n
    ctx.srs_generate(max(n, 1), 0, TAU)
    polys = _mixed(count, log_n)
    d = _dev(polys)
    proofs, evals = _open_batch(ctx, d, count, log_n)
    want_p, want_e = _singles(ctx, polys, count, log_n)
    assert proofs.shape == (count * n, 8) and np.array_equal(proofs, want_p), (log_n, count)
    assert np.array_equal(evals, want_e), (log_n, count)
    assert np.array_equal(_host(d, 4), polys)                                             # the input is never written
    assert np.array_equal(_open_batch(ctx, d, count, log_n, evals=False)[0], want_p)      # and without evals_dev
    if log_n == 0:
        assert not proofs.any() and np.array_equal(evals, polys)                          # points at infinity, the evals copied


def test_values_route(ctx):
    log_n, count, n = 6, 5, 64
    ctx.srs_generate(n, 0, TAU)
    ctx.srs_lagrange_clear()                                                              # this route reads no Lagrange-form key
    polys = _mixed(count, log_n, seed=11)
    vals = np.concatenate([ol.ntt(polys[b * n:(b + 1) * n], log_n) for b in range(count)])
    d_vals = _dev(vals)
    by_coeffs, ev_c = _open_batch(ctx, _dev(polys), count, log_n)
    by_values, ev_v = _open_batch(ctx, d_vals, count, log_n, values=True)
    assert np.array_equal(by_values, by_coeffs)
    assert np.array_equal(_host(d_vals, 4), vals)                                         # the input is unchanged
    assert np.array_equal(ev_c, vals) and np.array_equal(ev_v, vals)
    want_p, want_e = _singles(ctx, vals, count, log_n, values=True)
    assert np.array_equal(by_values, want_p) and np.array_equal(ev_v, want_e)
    assert np.array_equal(_open_batch(ctx, d_vals, count, log_n, values=True, evals=False)[0], by_coeffs)


# ------------------------------------------------------------------------------------------------ one independent referee
def test_every_proof_against_the_trapdoor(ctx):
    log_n, count, n = 5, 3, 32
    ctx.srs_generate(n - 1, 0, TAU)                                                       # N - 1 points: exactly what the pass reads
    polys = _rand_fr(count * n, 45)
    proofs, evals = _open_batch(ctx, _dev(polys), count, log_n)
    for b in range(count):
        want, vals = _trapdoor_proofs(polys[b * n:(b + 1) * n], log_n, TAU)
        assert np.array_equal(proofs[b * n:(b + 1) * n], want), b
        assert np.array_equal(evals[b * n:(b + 1) * n], vals), b


# ------------------------------------------------------------------------------------------------ verification
def test_all_openings_verify_and_none_after_the_polynomials_changed(ctx):
    import torch
    import plonkit_amd as pa
    log_n, count, n = 6, 3, 64
    total = count * n
    ctx.srs_generate(n, 0, TAU)
    polys = _rand_fr(total, 89)
    d = _dev(polys)
    cms = [ctx.kzg_commit_dev([_dev(polys[b * n:(b + 1) * n])], n)[0] for b in range(count)]
    d_cm = _dev(np.concatenate([np.tile(cm, (n, 1)) for cm in cms]))
    d_z = _dev(np.tile(ol.vpowers(ol.omega(log_n), n), (count, 1)))
    for changed, want in ((False, 1), (True, 0)):
        if changed:                                                                       # one coefficient of each polynomial moves, the commitments stay
            other = polys.copy()
            for b in range(count):
                k = b * n + 5 + b
                other[k] = ol.fr_mont(ol.fr_ints(polys[k:k + 1])[0] + 1)
            d = _dev(other)
        d_proofs, d_evals = _dev(np.zeros((total, 8), dtype=np.uint64)), _dev(np.zeros((total, 4), dtype=np.uint64))
        ctx.kzg_open_all_batch_dev(d, count, log_n, d_proofs, evals_ptr=d_evals)
        verdict = torch.full((total,), 0xAA, dtype=torch.uint8, device="cuda:0")
        ctx.kzg_verify_many_dev(d_cm, d_z, d_evals, d_proofs, total, pa.crs42_g2_bytes(), verdict)
        torch.cuda.synchronize()
        ctx.synchronize()
        assert (verdict.cpu().numpy() == want).all(), changed


# ------------------------------------------------------------------------------------------------ the kept transform of the key is one
def test_the_kept_transform_is_one_and_follows_the_key(ctx):
    log_n, count, n = 5, 2, 32
    polys = _rand_fr(count * n, 56)
    d, d0 = _dev(polys), _dev(polys[:n])
    want = np.concatenate([_trapdoor_proofs(polys[b * n:(b + 1) * n], log_n, TAU)[0] for b in range(count)])
    ctx.set_kernel_timing(True)
    try:
        ctx.srs_generate(n, 0, TAU)                                                       # voids whatever was kept
        single = _open_single(ctx, d0, log_n)[0]                                          # the single call builds the transform ..
        built_ms = ctx.kzg_open_all_last_ms()[0]
        batch = _open_batch(ctx, d, count, log_n)[0]                                      # .. and the batch call finds it
        kept_ms = ctx.kzg_open_all_last_ms()[0]
        print("key transform: built by the single call %.4f ms, kept for the batch call %.4f ms" % (built_ms, kept_ms))
        assert np.array_equal(single, want[:n]) and np.array_equal(batch, want)
        assert built_ms > KEPT_MS and kept_ms < KEPT_MS, (built_ms, kept_ms)
        ctx.srs_generate(n, 0, TAU)                                                       # the same key again: void for both
        batch = _open_batch(ctx, d, count, log_n)[0]                                      # the batch call builds ..
        built_ms = ctx.kzg_open_all_last_ms()[0]
        single = _open_single(ctx, d0, log_n)[0]                                          # .. and the single call finds it
        kept_ms = ctx.kzg_open_all_last_ms()[0]
        print("key transform: built by the batch call %.4f ms, kept for the single call %.4f ms" % (built_ms, kept_ms))
        assert np.array_equal(single, want[:n]) and np.array_equal(batch, want)
        assert built_ms > KEPT_MS and kept_ms < KEPT_MS, (built_ms, kept_ms)
    finally:
        ctx.set_kernel_timing(False)
    tau2 = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80912 % R_MOD
    ctx.srs_generate_fr(n, 0, ol.fr_mont(tau2))                                           # another tau, same size: a stale transform fails here
    moved = _open_batch(ctx, d, count, log_n)[0]
    assert np.array_equal(moved, np.concatenate([_trapdoor_proofs(polys[b * n:(b + 1) * n], log_n, tau2)[0] for b in range(count)]))
    assert not np.array_equal(moved, want)
    ctx.srs_generate(n, 0, TAU)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_themselves(ctx):
    import plonkit_amd as pa
    log_n, count, n = 4, 3, 16
    who, who_g1 = "plk_kzg_open_all_batch_dev", "plk_g1_ntt_batch_dev"
    polys = _rand_fr(count * n, 6)
    d, d_proofs, d_evals = _dev(polys), _dev(np.zeros((count * n, 8), dtype=np.uint64)), _dev(np.zeros((count * n, 4), dtype=np.uint64))
    batch = ctx.kzg_open_all_batch_dev

    def refused(code, words, f, *a, **kw):
        with pytest.raises(pa.PlkError) as e:
            f(*a, **kw)
        assert e.value.code == code and words in str(e.value), e.value

    ctx.srs_generate(n - 2, 0, TAU)                                                       # a key of N - 2 points
    refused(ERR_SRS, who + ": the pass reads key points 0 .. N - 2", batch, d, count, log_n, d_proofs)
    ctx.srs_generate(n - 1, 0, TAU)
    want = _open_batch(ctx, d, count, log_n)                                              # N - 1 points are enough
    refused(ERR_ARG, who + ": count must be at least 1", batch, d, 0, log_n, d_proofs)
    refused(ERR_SIZE, who + ": more than 2^25 points", batch, d, 1, 26, d_proofs)
    refused(ERR_SIZE, who + ": count x 2N exceeds 2^26 points", batch, d, 2, 25, d_proofs)     # the size is refused ahead of the short key
    refused(ERR_SIZE, who + ": count x 2N exceeds 2^26 points", batch, d, (1 << 14) + 1, 12, d_proofs)
    refused(ERR_ARG, who + ": device pointers must be 16-byte aligned", batch, d.data_ptr() + 8, count, log_n - 1, d_proofs)
    refused(ERR_ARG, who + ": device pointers must be 16-byte aligned", batch, d, count, log_n, d_proofs.data_ptr() + 8)
    refused(ERR_ARG, who + ": device pointers must be 16-byte aligned", batch, d, count, log_n, d_proofs, evals_ptr=d_evals.data_ptr() + 8)
    refused(ERR_ARG, who + ": bad argument", batch, 0, count, log_n, d_proofs)
    refused(ERR_ARG, who + ": bad argument", batch, d, count, log_n, d_proofs, evals_ptr=d)
    refused(ERR_ARG, who_g1 + ": count must be at least 1", ctx.g1_ntt_batch_dev, d_proofs, 0, log_n, d_proofs)
    refused(ERR_ARG, who_g1 + ": device pointers must be 16-byte aligned", ctx.g1_ntt_batch_dev, d_proofs.data_ptr() + 8, 1, log_n, d_proofs)
    refused(ERR_SIZE, who_g1 + ": size exceeds 2^26", ctx.g1_ntt_batch_dev, d_proofs, 65, 20, d_proofs)
    refused(ERR_SIZE, who_g1 + ": size exceeds 2^26", ctx.g1_ntt_batch_dev, d_proofs, 1, 27, d_proofs)
    ctx.set_commit_shard(0, lambda partial: None)                                         # a context that holds one shard of a key
    try:
        refused(ERR_ARG, who + ": single-GPU only", batch, d, count, log_n, d_proofs)
    finally:
        ctx.set_commit_shard(0, None)
    ctx.srs_generate(n, 0, TAU)
    ctx.msm_enqueue_dev(d, n)                                                             # a commitment in flight
    try:
        refused(ERR_ARG, who + ": a commitment is still in flight on this context", batch, d, count, log_n, d_proofs)
        refused(ERR_ARG, who_g1 + ": a commitment enqueued with plk_msm_g1_enqueue_dev is still in flight", ctx.g1_ntt_batch_dev, d_proofs, count, log_n, d_proofs)
    finally:
        ctx.msm_finish()
    again = _open_batch(ctx, d, count, log_n)                                             # and the context still works
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    ctx.srs_generate(1 << 12, 0, TAU)                                                     # (12, 1) on the context that refused (12, 2^14 + 1)
    big = _rand_fr(1 << 12, 12)
    refused(ERR_SIZE, who + ": count x 2N exceeds 2^26 points", batch, _dev(big), (1 << 14) + 1, 12, d_proofs)
    proofs, evals = _open_batch(ctx, _dev(big), 1, 12)
    one_p, one_e = _open_single(ctx, _dev(big), 12)
    assert np.array_equal(proofs, one_p) and np.array_equal(evals, one_e)
