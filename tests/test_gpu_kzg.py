"""-m gpu: KZG openings on their own (kzg.hip): evaluation and division from the values on the domain, commitments in either form,
plk_kzg_open_dev by both routes, and plk_kzg_verify_many_dev against plk_kzg_verify.

Referees.  The two values helpers: the oracle's C routines through the coefficient route (ol.ntt inverse -> ol.poly_eval /
ol.poly_div_linear -> ol.ntt), and below 2^5 the Python-integer model of tests/gen/kzg_cases.py as well.  Commitments and proofs: the
trapdoor of the tau = 42 key — C = f(42) G and pi = ((F(42) - F(z)) / (42 - z)) G by ol.poly_eval and ol.g1_mul, no CPU MSM — and where
z = 42 (or the key is at most 2^10 points) the oracle's ol.msm over the downloaded key.  Verdicts: plk_kzg_verify on the same opening."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol
from oracle.oracle_lib import Q_MOD, R_MOD
from tests.gen import kzg_cases as kc

ERR_ARG, ERR_SRS = 1, 3
TAU = 42
TOP = 0x30644e72e131a029                                        # top limb of r: four limbs with a smaller top one are a residue


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _host(t, width=4):
    return t.cpu().numpy().view(np.uint64).reshape(-1, width)


def _rand_fr(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, TOP, size=n, dtype=np.uint64)
    return a


def _values(kind, log_n, z, seed):
    n = 1 << log_n
    if kind == "zero":
        return np.zeros((n, 4), dtype=np.uint64)
    if kind == "constant":
        return np.tile(ol.fr_mont(7), (n, 1))
    if kind == "all_r_minus_1":
        return np.tile(ol.fr_mont(R_MOD - 1), (n, 1))
    if kind == "x_minus_z":
        return ol.vadd_scalar(ol.vpowers(ol.omega(log_n), n), (-z) % R_MOD)
    return _rand_fr(n, seed)


def _reference(vals, log_n, z):
    """(f(z), the values of (f - f(z)) / (x - z)) through the coefficient route of the oracle's C routines"""
    coeffs = ol.ntt(vals, log_n, inverse=True)
    return ol.poly_eval(coeffs, z), ol.ntt(ol.poly_div_linear(coeffs, z), log_n)


# ------------------------------------------------------------------------------------------------ the two values helpers
@pytest.mark.parametrize("log_n", kc.HELPER_LOG_NS)
def test_values_helpers(ctx, log_n):
    n = 1 << log_n
    for zi, (zname, z) in enumerate(kc.z_cases(log_n).items()):
        zm = ol.fr_mont(z)
        for ki, kind in enumerate(kc.POLY_KINDS):
            what = (log_n, zname, kind)
            vals = _values(kind, log_n, z, 100 * zi + ki)
            y_ref, q_ref = _reference(vals, log_n, z)
            d_in, d_out = _dev(vals), _dev(np.zeros((n, 4), dtype=np.uint64))
            y = ctx.poly_evaluate_values_at_dev(d_in, log_n, zm)
            assert np.array_equal(y, ol.fr_mont(y_ref)), what
            ctx.poly_divide_values_by_linear_dev(d_in, log_n, zm, d_out)
            assert np.array_equal(_host(d_out), q_ref), what
            assert np.array_equal(_host(d_in), vals), what                            # the input is never written
            if kind == "x_minus_z":
                assert y_ref == 0 and np.array_equal(q_ref, np.tile(ol.fr_mont(1), (n, 1))), what
            if log_n in kc.MODEL_LOG_NS:                                              # the Python-integer model as a second referee
                ints = ol.fr_ints(vals)
                assert y_ref == kc.evaluate_values(ints, log_n, z) and ol.fr_ints(q_ref) == kc.quotient_values(ints, log_n, z), what
            if kind == "random":
                # a caller's y, and the output over the input
                ctx.poly_divide_values_by_linear_dev(d_in, log_n, zm, d_in, y=ol.fr_mont(y_ref))
                assert np.array_equal(_host(d_in), q_ref), what


def test_a_callers_y_is_taken_on_trust_outside_the_domain_and_checked_inside(ctx):
    import plonkit_amd as pa
    log_n, n = 12, 1 << 12
    vals = _rand_fr(n, 7)
    d_in, d_out = _dev(vals), _dev(np.zeros((n, 4), dtype=np.uint64))
    z = kc.z_cases(log_n)["random"]
    y = 123456789
    ctx.poly_divide_values_by_linear_dev(d_in, log_n, ol.fr_mont(z), d_out, y=ol.fr_mont(y))
    dom = ol.vpowers(ol.omega(log_n), n)
    want = ol.vmul(ol.vadd_scalar(vals, (-y) % R_MOD), ol.vbatch_inv(ol.vadd_scalar(dom, (-z) % R_MOD)))
    assert np.array_equal(_host(d_out), want)
    for k in (0, 2047, 2048, n - 1):
        zk = ol.fr_mont(pow(ol.omega(log_n), k, R_MOD))
        fk = ol.fr_ints(vals[k:k + 1])[0]
        with pytest.raises(pa.PlkError) as e:
            ctx.poly_divide_values_by_linear_dev(d_in, log_n, zk, d_out, y=ol.fr_mont(fk + 1))
        assert e.value.code == ERR_ARG and "omega^%d" % k in str(e.value)
        ctx.poly_divide_values_by_linear_dev(d_in, log_n, zk, d_out, y=ol.fr_mont(fk))       # the right value is accepted
        assert np.array_equal(_host(d_out), _reference(vals, log_n, pow(ol.omega(log_n), k, R_MOD))[1])


def test_values_helpers_past_one_launch_of_block_totals(ctx):
    """2^22 elements are 2048 scan blocks: more than the 1024 lanes of the totals scan hold one each"""
    log_n, n = kc.LARGE_LOG_N, 1 << kc.LARGE_LOG_N
    vals = _rand_fr(n, 22)
    coeffs = ol.ntt(vals, log_n, inverse=True)
    d_in, d_out = _dev(vals), _dev(np.zeros((n, 4), dtype=np.uint64))
    for z in (kc.z_cases(log_n)["random"], pow(ol.omega(log_n), (1 << 21) + 5, R_MOD)):
        y = ctx.poly_evaluate_values_at_dev(d_in, log_n, ol.fr_mont(z))
        assert np.array_equal(y, ol.fr_mont(ol.poly_eval(coeffs, z)))
        ctx.poly_divide_values_by_linear_dev(d_in, log_n, ol.fr_mont(z), d_out)
        assert np.array_equal(_host(d_out), ol.ntt(ol.poly_div_linear(coeffs, z), log_n))


# ------------------------------------------------------------------------------------------------ commitments and openings
G = ol.g1_generator()


def _g(k):
    return ol.g1_mul(G, k % R_MOD) if k % R_MOD else np.zeros(8, dtype=np.uint64)


def _trapdoor_opening(coeff_list, z, v):
    """(commitments, evals as ints, proof) from tau = 42; z != 42"""
    at_tau = [ol.poly_eval(c, TAU) for c in coeff_list]
    at_z = [ol.poly_eval(c, z) for c in coeff_list]
    F_tau = sum(pow(v, j, R_MOD) * a for j, a in enumerate(at_tau)) % R_MOD
    F_z = sum(pow(v, j, R_MOD) * a for j, a in enumerate(at_z)) % R_MOD
    return np.stack([_g(a) for a in at_tau]), at_z, _g((F_tau - F_z) * pow(TAU - z, -1, R_MOD))


def _key(ctx, log_n):
    ctx.srs_generate(1 << log_n, 0, TAU)
    ctx.srs_lagrange_from_powers(log_n)


@pytest.mark.parametrize("log_n", [1, 2, 3, 8, 11, 12])
def test_open_both_routes_agree_with_each_other_and_the_trapdoor(ctx, log_n):
    n = 1 << log_n
    _key(ctx, log_n)
    key = ctx.srs_download(0, n)
    vals = [_rand_fr(n, 10 * log_n + j) for j in range(8)]
    vals[5] = np.zeros((n, 4), dtype=np.uint64)                                       # the zero polynomial among the others
    coeffs = [ol.ntt(a, log_n, inverse=True) for a in vals]
    d_vals, d_coeffs = [_dev(a) for a in vals], [_dev(a) for a in coeffs]
    v = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100abcd % R_MOD
    cm_c, cm_v = ctx.kzg_commit_dev(d_coeffs, n), ctx.kzg_commit_dev(d_vals, n, values=True)
    assert np.array_equal(cm_c, cm_v) and np.array_equal(cm_c, ctx.msm_batch_dev(d_coeffs, n))
    assert np.array_equal(cm_c, np.stack([_g(ol.poly_eval(c, TAU)) for c in coeffs]))
    for zname, z in kc.z_cases(log_n).items():
        for count in (1, 2, 8):
            what = (log_n, zname, count)
            vm = ol.fr_mont(v) if count > 1 else None
            ev_c, pi_c = ctx.kzg_open_dev(d_coeffs[:count], n, ol.fr_mont(z), v=vm)
            ev_v, pi_v = ctx.kzg_open_dev(d_vals[:count], n, ol.fr_mont(z), v=vm, values=True)
            assert np.array_equal(ev_c, ev_v) and np.array_equal(pi_c, pi_v), what
            assert ol.fr_ints(ev_c) == [ol.poly_eval(c, z) for c in coeffs[:count]], what
            if z != TAU:
                cms, _, pi = _trapdoor_opening(coeffs[:count], z, v)
                assert np.array_equal(pi_c, pi), what
                assert np.array_equal(cms, cm_c[:count]), what
            if log_n <= 10 or z == TAU:                                               # the oracle's MSM as a second referee (the only one at z = 42)
                F = coeffs[0]
                for j in range(1, count):
                    F = ol.vaxpy(F, pow(v, j, R_MOD), coeffs[j])
                assert np.array_equal(pi_c, ol.msm(key, ol.poly_div_linear(F, z))), what
    for a, d in zip(vals + coeffs, d_vals + d_coeffs):
        assert np.array_equal(_host(d), a)                                            # the inputs are what they were


def test_open_verifies_on_the_host(ctx):
    import plonkit_amd as pa
    log_n, n = 8, 256
    _key(ctx, log_n)
    d_vals = [_dev(_rand_fr(n, 800 + j)) for j in range(3)]
    cms = ctx.kzg_commit_dev(d_vals, n, values=True)
    v = ol.fr_mont(987654321)
    for zname, z in kc.z_cases(log_n).items():
        evals, proof = ctx.kzg_open_dev(d_vals, n, ol.fr_mont(z), v=v, values=True)
        assert pa.kzg_verify(cms, ol.fr_mont(z), evals, proof, pa.crs42_g2_bytes(), v=v) is True, zname
        evals[1] = ol.fr_mont(ol.fr_ints(evals[1:2])[0] + 1)
        assert pa.kzg_verify(cms, ol.fr_mont(z), evals, proof, pa.crs42_g2_bytes(), v=v) is False, zname


@pytest.mark.parametrize("n", [1, 2047, 2049])
def test_open_coefficients_of_any_length_and_at_zero(ctx, n):
    ctx.srs_generate(4096, 0, TAU)
    coeffs = [_rand_fr(n, 3 * n + j) for j in range(2)]
    d = [_dev(a) for a in coeffs]
    v = 31337
    for z in (0, 1, kc.z_cases(12)["random"], R_MOD - 1):
        for count in (1, 2):
            evals, proof = ctx.kzg_open_dev(d[:count], n, ol.fr_mont(z), v=ol.fr_mont(v))
            cms, at_z, pi = _trapdoor_opening(coeffs[:count], z, v)
            assert ol.fr_ints(evals) == at_z and np.array_equal(proof, pi), (n, z, count)
            if z == 0:
                assert at_z == [ol.fr_ints(c[:1])[0] for c in coeffs[:count]]         # y = c_0
    for a, t in zip(coeffs, d):
        assert np.array_equal(_host(t), a)


def test_refusals(ctx):
    import plonkit_amd as pa
    log_n, n = 8, 256
    ctx.srs_generate(n, 0, TAU)
    ctx.srs_lagrange_clear()
    d = _dev(_rand_fr(n, 5))
    z = ol.fr_mont(5)

    def refused(code, words, f, *a, **kw):
        with pytest.raises(pa.PlkError) as e:
            f(*a, **kw)
        assert e.value.code == code and words in str(e.value), e.value

    size_words = "Lagrange-form key has a different size than the circuit's domain"
    refused(ERR_SRS, size_words, ctx.kzg_open_dev, [d], n, z, values=True)            # no Lagrange-form key
    refused(ERR_SRS, size_words, ctx.kzg_commit_dev, [d], n, values=True)
    ctx.srs_lagrange_from_powers(log_n - 1)                                           # one of another size
    refused(ERR_SRS, size_words, ctx.kzg_open_dev, [d], n, z, values=True)
    refused(ERR_SRS, size_words, ctx.kzg_commit_dev, [d], n, values=True)
    ctx.srs_lagrange_from_powers(log_n)
    ctx.msm_enqueue_dev(d, n)                                                         # a commitment in flight
    try:
        refused(ERR_ARG, "a commitment is still in flight on this context", ctx.kzg_open_dev, [d], n, z)
        refused(ERR_ARG, "a commitment is still in flight on this context", ctx.kzg_open_dev, [d], n, z, values=True)
    finally:
        ctx.msm_finish()
    refused(ERR_ARG, "bad argument", ctx.kzg_open_dev, [0], n, z)                     # null pointers
    refused(ERR_ARG, "bad argument", ctx.kzg_open_dev, [d, d], n, z)                  # two polynomials, no v
    refused(ERR_ARG, "bad argument", ctx.kzg_open_dev, [d] * 9, n, z, v=z)
    refused(ERR_ARG, "bad argument", ctx.kzg_commit_dev, [0], n)
    refused(ERR_ARG, "bad argument", ctx.poly_evaluate_values_at_dev, 0, log_n, z)
    refused(ERR_ARG, "bad argument", ctx.poly_evaluate_values_at_dev, d, 0, z)
    refused(ERR_ARG, "bad argument", ctx.poly_evaluate_values_at_dev, d, 29, z)
    refused(ERR_ARG, "bad argument", ctx.poly_divide_values_by_linear_dev, d, log_n, z, 0)
    refused(ERR_ARG, "bad argument", ctx.poly_evaluate_values_at_dev, d, log_n, ol.int_to_limbs(R_MOD))      # z = r
    evals, proof = ctx.kzg_open_dev([d], n, z, values=True)                           # and the context still works
    assert np.array_equal(proof, ctx.kzg_open_dev([_dev(ol.ntt(_host(d), log_n, inverse=True))], n, z)[1])


# ------------------------------------------------------------------------------------------------ many openings on the device
def _opening_kinds():
    """eight openings by construction (tau = 42): valid, each part tampered singly, infinity commitment and proof, infinity proof, malformed"""
    rng = np.random.default_rng(99)
    out = []
    for kind in range(10):
        c = [int(x) for x in rng.integers(1, 1 << 62, size=5)]
        z = int(rng.integers(1 << 20, 1 << 62))
        f_tau, f_z = kc.horner(c, TAU), kc.horner(c, z)
        C, y, pi = _g(f_tau), f_z, _g((f_tau - f_z) * pow(TAU - z, -1, R_MOD))
        zl, yl = ol.fr_mont(z), ol.fr_mont(y)
        if kind == 1:
            zl = ol.fr_mont(z + 1)
        elif kind == 2:
            yl = ol.fr_mont(y + 1)
        elif kind == 3:
            pi = ol.g1_add(pi, G)
        elif kind == 4:
            C = ol.g1_add(C, G)
        elif kind == 5:                                                               # the zero polynomial
            C, yl, pi = np.zeros(8, dtype=np.uint64), ol.fr_mont(0), np.zeros(8, dtype=np.uint64)
        elif kind == 6:                                                               # a constant: infinity proof
            C, yl, pi = _g(7), ol.fr_mont(7), np.zeros(8, dtype=np.uint64)
        elif kind == 7:                                                               # off the curve
            C = C.copy(); C[4] ^= np.uint64(1)
        elif kind == 8:                                                               # a scalar that is no residue
            yl = ol.int_to_limbs(R_MOD)
        elif kind == 9:                                                               # a coordinate that is no residue
            pi = pi.copy(); pi[:4] = ol.int_to_limbs(Q_MOD + 1)
        out.append((C, zl, yl, pi))
    return out


@pytest.fixture(scope="module")
def kinds():
    import plonkit_amd as pa
    ks, want = _opening_kinds(), []
    for C, zl, yl, pi in ks:
        try:
            want.append(1 if pa.kzg_verify(C[None], zl, yl[None], pi, pa.crs42_g2_bytes()) else 0)
        except pa.PlkError as e:
            assert e.code == ERR_ARG
            want.append(2)
    assert want == [1, 0, 0, 0, 0, 1, 1, 2, 2, 2]                                     # what the construction says
    return ks, want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_verify_many_is_kzg_verify_per_opening(ctx, kinds, n):
    import torch
    import plonkit_amd as pa
    ks, want = kinds
    order = [(3 * i + i // 10) % 10 for i in range(n)]                                # malformed entries between valid and invalid ones
    if n == 1:
        order = [0]
    cols = [np.stack([ks[k][j] for k in order]) if n else np.zeros((0, w), dtype=np.uint64) for j, w in enumerate((8, 4, 4, 8))]
    d = [_dev(c) if n else 0 for c in cols]
    verdict = torch.full((n + 48,), 0xAA, dtype=torch.uint8, device="cuda:0")
    ctx.kzg_verify_many_dev(d[0], d[1], d[2], d[3], n, pa.crs42_g2_bytes(), verdict.data_ptr() + 16 if n else 0)
    torch.cuda.synchronize()
    ctx.synchronize()
    got = verdict.cpu().numpy()
    assert list(got[16:16 + n]) == [want[k] for k in order]
    assert (got[:16] == 0xAA).all() and (got[16 + n:] == 0xAA).all()                  # canaries on both sides


def test_verify_many_refusals(ctx, kinds):
    import plonkit_amd as pa
    ks, _ = kinds
    d = [_dev(np.stack([k[j] for k in ks])) for j in range(4)]
    out = _dev(np.zeros((2, 4), dtype=np.uint64))
    bad = bytearray(pa.crs42_g2_bytes()); bad[255] ^= 1
    with pytest.raises(pa.PlkError) as e:
        ctx.kzg_verify_many_dev(d[0], d[1], d[2], d[3], len(ks), bytes(bad), out)
    assert e.value.code == ERR_ARG and "plk_pairing_check: G2 point not on the twist" in str(e.value)
    with pytest.raises(pa.PlkError) as e:
        ctx.kzg_verify_many_dev(d[0], 0, d[2], d[3], len(ks), pa.crs42_g2_bytes(), out)
    assert e.value.code == ERR_ARG
