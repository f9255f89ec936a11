"""-m gpu: the openings at all points of the domain in one pass (kzg_all.hip: plk_kzg_open_all_dev, _prepare) and the G1 transform in both
directions (g1ntt.hip: plk_g1_ntt_dev).

Referees.  The transform: ol.ntt on the discrete logarithms, then ol.g1_mul.  The proofs: up to 2^4 plk_kzg_open_dev at every omega^i from the
same coefficients; at 2^7, 2^8 and 2^10 (the 2N-point transform on and above the 2^8 re-indexing seam of g1ntt_stage) the trapdoor of the
tau = 42 key, pi_i = ((f(42) - f(omega^i)) / (42 - omega^i)) G by ol.ntt, ol.vbatch_inv and ol.g1_mul, no CPU MSM; the verdicts of
plk_kzg_verify_many_dev.  Affine coordinates are unique: every comparison is an equality of bytes."""
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


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


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


def _open_all(ctx, d_poly, log_n, values=False, evals=False):
    n = 1 << log_n
    d_proofs = _dev(np.full((n, 8), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64))
    d_evals = _dev(np.full((n, 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)) if evals else None
    ctx.kzg_open_all_dev(d_poly, log_n, d_proofs, evals_ptr=d_evals, values=values)
    return (_host(d_proofs, 8), _host(d_evals, 4)) if evals else _host(d_proofs, 8)


def _trapdoor_proofs(coeffs, log_n, tau):
    """every pi_i from the secret: ((f(omega^i) - f(tau)) / (omega^i - tau)) G; also the values f(omega^i)"""
    n = 1 << log_n
    vals = ol.ntt(coeffs, log_n)
    num = ol.vadd_scalar(vals, -ol.poly_eval(coeffs, tau))
    den = ol.vbatch_inv(ol.vadd_scalar(ol.vpowers(ol.omega(log_n), n), -tau))
    return _points(ol.fr_ints(ol.vmul(num, den))), vals


def _coeffs(kind, log_n, seed=3):
    return ol.fr_vec(fk.poly(kind, log_n, seed))


# ------------------------------------------------------------------------------------------------ the G1 transform, forward and back
def _ntt_inputs(kind, log_n):
    n = 1 << log_n
    rng = np.random.default_rng(50 + log_n)
    if kind == "equal":                                                                   # every output but the first is the identity
        return [123456789] * n
    if kind == "spike":                                                                   # a_j = omega^j: one non-zero output, at N - 1
        return ol.fr_ints(ol.vpowers(ol.omega(log_n), n))
    a = ol.fr_ints(_rand_fr(n, 700 + log_n))
    if kind == "identities":
        for j in rng.choice(n, size=(n + 2) // 3, replace=False):
            a[int(j)] = 0
        a[0] = 0
    return a


@pytest.mark.parametrize("log_n", [1, 2, 5, 6, 7, 8, 9])
def test_g1_ntt_forward_against_the_scalar_transform(ctx, log_n):
    n = 1 << log_n
    for kind in ("random", "equal", "identities", "spike"):
        a = _ntt_inputs(kind, log_n)
        pts = _points(a)
        want_logs = ol.fr_ints(ol.ntt(ol.fr_vec(a), log_n))
        if kind == "equal":
            assert want_logs[0] and not any(want_logs[1:])
        if kind == "spike":
            assert want_logs[n - 1] and sum(1 for v in want_logs if v) == 1
        d_in, d_out, d_back = _dev(pts), _dev(np.zeros((n, 8), dtype=np.uint64)), _dev(np.zeros((n, 8), dtype=np.uint64))
        ctx.g1_ntt_dev(d_in, log_n, d_out)
        ctx.g1_ntt_dev(d_out, log_n, d_back, inverse=True)
        ctx.synchronize()
        assert np.array_equal(_host(d_out, 8), _points(want_logs)), (log_n, kind)
        assert np.array_equal(_host(d_back, 8), pts), (log_n, kind)                      # the round trip returns the input bytes
        assert np.array_equal(_host(d_in, 8), pts), (log_n, kind)
        if kind in ("random", "identities"):                                              # inverse = 1 is plk_g1_intt
            ctx.g1_ntt_dev(d_in, log_n, d_out, inverse=True)
            ctx.synchronize()
            assert np.array_equal(_host(d_out, 8), ctx.g1_intt(pts, log_n)), (log_n, kind)


# ------------------------------------------------------------------------------------------------ the proofs
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4])
def test_every_proof_is_plk_kzg_open_devs(ctx, log_n):
    n = 1 << log_n
    ctx.srs_generate(max(n, 1), 0, TAU)
    w = ol.omega(log_n)
    for kind in fk.POLY_KINDS:
        coeffs = _coeffs(kind, log_n)
        d = _dev(coeffs)
        proofs, evals = _open_all(ctx, d, log_n, evals=True)
        assert proofs.shape == (n, 8)
        for i in range(n):
            ev, pi = ctx.kzg_open_dev([d], n, ol.fr_mont(pow(w, i, R_MOD)))
            assert np.array_equal(proofs[i], pi), (log_n, kind, i)
            assert np.array_equal(evals[i], ev[0]), (log_n, kind, i)
        if kind in ("zero", "constant") or log_n == 0:
            assert not proofs.any(), (log_n, kind)                                        # the point at infinity
        assert np.array_equal(_host(d, 4), coeffs)                                        # the input is never written


@pytest.mark.parametrize("log_n", [7, 8, 10])
def test_every_proof_against_the_trapdoor(ctx, log_n):
    n = 1 << log_n
    ctx.srs_generate(n - 1, 0, TAU)                                                       # N - 1 points: exactly what the pass reads
    coeffs = _rand_fr(n, 40 + log_n)
    want, vals = _trapdoor_proofs(coeffs, log_n, TAU)
    proofs, evals = _open_all(ctx, _dev(coeffs), log_n, evals=True)
    assert np.array_equal(proofs, want)
    assert np.array_equal(evals, vals)


def test_values_route(ctx):
    log_n, n = 6, 64
    ctx.srs_generate(n, 0, TAU)
    ctx.srs_lagrange_clear()                                                              # this route reads no Lagrange-form key
    coeffs = _rand_fr(n, 66)
    vals = ol.ntt(coeffs, log_n)
    d_vals = _dev(vals)
    by_coeffs, ev_c = _open_all(ctx, _dev(coeffs), log_n, evals=True)
    by_values, ev_v = _open_all(ctx, d_vals, log_n, values=True, evals=True)
    assert np.array_equal(by_values, by_coeffs)
    assert np.array_equal(_host(d_vals, 4), vals)                                         # the input is unchanged
    assert np.array_equal(ev_c, vals) and np.array_equal(ev_v, vals)
    assert np.array_equal(by_coeffs, _trapdoor_proofs(coeffs, log_n, TAU)[0])
    assert np.array_equal(_open_all(ctx, d_vals, log_n, values=True), by_coeffs)          # and without evals_dev


def test_all_openings_verify_and_none_after_the_polynomial_changed(ctx):
    import torch
    import plonkit_amd as pa
    log_n, n = 8, 256
    ctx.srs_generate(n, 0, TAU)
    coeffs = _rand_fr(n, 88)
    d = _dev(coeffs)
    cm = ctx.kzg_commit_dev([d], n)[0]
    d_cm, d_z = _dev(np.tile(cm, (n, 1))), _dev(ol.vpowers(ol.omega(log_n), n))
    for changed, want in ((False, 1), (True, 0)):
        if changed:                                                                       # one coefficient moves, the commitment stays
            other = coeffs.copy()
            other[5] = ol.fr_mont(ol.fr_ints(coeffs[5:6])[0] + 1)
            d = _dev(other)
        d_proofs, d_evals = _dev(np.zeros((n, 8), dtype=np.uint64)), _dev(np.zeros((n, 4), dtype=np.uint64))
        ctx.kzg_open_all_dev(d, log_n, d_proofs, evals_ptr=d_evals)
        verdict = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda:0")
        ctx.kzg_verify_many_dev(d_cm, d_z, d_evals, d_proofs, n, pa.crs42_g2_bytes(), verdict)
        torch.cuda.synchronize()
        ctx.synchronize()
        assert (verdict.cpu().numpy() == want).all(), changed


# ------------------------------------------------------------------------------------------------ the cached transform of the key
def test_the_keys_transform_is_kept_and_follows_the_key(ctx):
    log_n, n = 5, 32
    coeffs = _rand_fr(n, 55)
    d = _dev(coeffs)
    ctx.srs_generate(n, 0, TAU)
    alone = _open_all(ctx, d, log_n)                                                      # builds the transform on the way
    assert np.array_equal(_open_all(ctx, d, log_n), alone)                                # and uses the kept one
    ctx.srs_generate(n, 0, TAU)                                                           # the same key again: the kept transform is void
    ctx.kzg_open_all_prepare(log_n)
    assert np.array_equal(_open_all(ctx, d, log_n), alone)
    assert np.array_equal(alone, _trapdoor_proofs(coeffs, log_n, TAU)[0])
    tau2 = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80912 % R_MOD
    ctx.srs_generate_fr(n, 0, ol.fr_mont(tau2))                                           # another tau on the same context, same size: a stale transform fails here
    moved = _open_all(ctx, d, log_n)
    assert np.array_equal(moved, _trapdoor_proofs(coeffs, log_n, tau2)[0])
    assert not np.array_equal(moved, alone)
    ctx.kzg_open_all_prepare(log_n - 1)                                                   # another size asked for in between
    assert np.array_equal(_open_all(ctx, d, log_n), moved)
    key = _dev(ctx.srs_download(0, n))                                                    # a caller's key in device memory (plk_srs_set_dev) will do
    ctx.srs_generate(n, 0, TAU)
    ctx.srs_set_dev(key, n)
    assert np.array_equal(_open_all(ctx, d, log_n), moved)
    ctx.srs_generate(n, 0, TAU)                                                           # (the context owns its key again before `key` goes)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_themselves(ctx):
    import plonkit_amd as pa
    log_n, n = 4, 16
    d, d_proofs = _dev(_rand_fr(n, 5)), _dev(np.zeros((n, 8), dtype=np.uint64))

    def refused(code, words, f, *a, **kw):
        with pytest.raises(pa.PlkError) as e:
            f(*a, **kw)
        assert e.value.code == code and words in str(e.value), e.value

    ctx.srs_generate(n - 2, 0, TAU)                                                       # a key of N - 2 points
    refused(ERR_SRS, "plk_kzg_open_all_dev", ctx.kzg_open_all_dev, d, log_n, d_proofs)
    refused(ERR_SRS, "plk_kzg_open_all_prepare", ctx.kzg_open_all_prepare, log_n)
    ctx.srs_generate(n - 1, 0, TAU)
    want = _open_all(ctx, d, log_n)                                                       # N - 1 points are enough
    refused(ERR_SIZE, "plk_kzg_open_all_dev: more than 2^25 points", ctx.kzg_open_all_dev, d, 26, d_proofs)
    refused(ERR_SIZE, "plk_kzg_open_all_prepare", ctx.kzg_open_all_prepare, 26)
    refused(ERR_ARG, "plk_kzg_open_all_dev: device pointers must be 16-byte aligned", ctx.kzg_open_all_dev, d.data_ptr() + 8, log_n - 1, d_proofs)
    refused(ERR_ARG, "plk_kzg_open_all_dev: device pointers must be 16-byte aligned", ctx.kzg_open_all_dev, d, log_n, d_proofs.data_ptr() + 8)
    refused(ERR_ARG, "plk_kzg_open_all_dev: bad argument", ctx.kzg_open_all_dev, 0, log_n, d_proofs)
    refused(ERR_ARG, "plk_kzg_open_all_dev: bad argument", ctx.kzg_open_all_dev, d, log_n, d_proofs, evals_ptr=d)
    refused(ERR_ARG, "plk_g1_ntt_dev: device pointers must be 16-byte aligned", ctx.g1_ntt_dev, d_proofs.data_ptr() + 8, log_n - 1, d_proofs)
    refused(ERR_SIZE, "plk_g1_ntt_dev: size exceeds 2^26", ctx.g1_ntt_dev, d_proofs, 27, d_proofs)
    refused(ERR_ARG, "plk_kzg_open_all_last_ms", ctx.kzg_open_all_last_ms)                # timing was never switched on
    ctx.srs_generate(n, 0, TAU)
    ctx.msm_enqueue_dev(d, n)                                                             # a commitment in flight
    try:
        refused(ERR_ARG, "plk_kzg_open_all_dev: a commitment is still in flight on this context", ctx.kzg_open_all_dev, d, log_n, d_proofs)
        refused(ERR_ARG, "plk_kzg_open_all_prepare: a commitment is still in flight on this context", ctx.kzg_open_all_prepare, log_n)
        refused(ERR_ARG, "plk_g1_ntt_dev: a commitment enqueued with plk_msm_g1_enqueue_dev is still in flight", ctx.g1_ntt_dev, d_proofs, log_n, d_proofs)
    finally:
        ctx.msm_finish()
    assert np.array_equal(_open_all(ctx, d, log_n), want)                                 # and the context still works
    ctx.set_kernel_timing(True)
    try:
        _open_all(ctx, d, log_n)
        ms = ctx.kzg_open_all_last_ms()
        assert len(ms) == 5 and all(v >= 0 for v in ms) and sum(ms[1:]) > 0
    finally:
        ctx.set_kernel_timing(False)
