"""-m gpu: the multi-point openings from values on the domain (kzg_multi_values.hip): plk_poly_evaluate_values_multi_dev,
plk_poly_quotient_multi_values_dev and plk_kzg_open_multi_values_dev against the Lagrange-form key.

Referees.  The oracle: ol.ntt(inverse) takes the values to coefficients, ol.poly_eval and the grouped formula through ol.poly_div_linear
work there (tests/test_gpu_kzg_multi.py: _quotient_ref, _model_opening), ol.ntt brings a quotient back to values.  The trapdoor of the
tau = 42 key: W = h(42) G and W' = Q(42) G.  The coefficient route plk_kzg_open_multi_dev on the oracle's coefficients, byte for byte.
Below N = 32 also the Python-integer model of tests/gen/kzg_multi_values_cases.py, which its host test holds against the definition.
Equality is exact everywhere: no tolerance.
THE TILE is the scan engine's 2048 elements: 2^1 and 2^3 are below one, 2^11 is one exactly, 2^12 two, 2^16 thirty-two with block prefixes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD
from tests.gen import kzg_multi_cases as km
from tests.gen import kzg_multi_values_cases as kv
from tests.test_gpu_kzg_multi import (GAMMA, TAU, TILE, U_RANDOM, _coef, _dev, _g, _host, _model_opening, _mont_list, _mont_matrix, _points, _quotient_ref,
                                      _rand_fr)

ERR_ARG, ERR_SRS, ERR_HIP, ERR_IO = 1, 3, 4, 7
LOG_SIZES = (1, 3, 11, 12, 16)
SIZE_WORDS = "Lagrange-form key has a different size than the circuit's domain"


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    c.srs_generate(1 << 16, 0, TAU)
    yield c
    c.close()


def _key(ctx, log_n):
    if ctx.srs_lagrange_size() != 1 << log_n:
        ctx.srs_lagrange_from_powers(log_n)


_DATA = {}


def _data(log_n, count):
    """(values, coefficients, device values, device coefficients) of `count` polynomials of 2^log_n values: computed once per size, never written"""
    have = _DATA.setdefault(log_n, ([], [], [], []))
    n = 1 << log_n
    while len(have[0]) < count:
        i = len(have[0])
        v = _rand_fr(n, 5000 * log_n + i)
        if i == 2:
            v = np.zeros((n, 4), dtype=np.uint64)                                     # a zero polynomial among the inputs
        if i == 4:
            v = np.tile(ol.fr_mont(R_MOD - 1), (n, 1))                                # every value r - 1 (the constant r - 1)
        c = ol.ntt(v, log_n, inverse=True)
        have[0].append(v); have[1].append(c); have[2].append(_dev(v)); have[3].append(_dev(c))
    return tuple(x[:count] for x in have)


def _values_of(coeffs, log_n):
    return ol.ntt(coeffs, log_n)


def _omega_pow(log_n, k):
    return pow(km.omega(log_n), k, R_MOD)


def _check_operator(ctx, log_n, vals, coeffs, d_vals, d_out, points, coef, what):
    """the quotient in values and the evaluations of the pairs with a non-zero coefficient, against the oracle's coefficients"""
    n = 1 << log_n
    ctx.poly_quotient_multi_values_dev(d_vals, log_n, _mont_list(points), _mont_matrix(coef), d_out)
    got = _host(d_out)
    assert np.array_equal(got, _values_of(_quotient_ref(coeffs, points, coef), log_n)), what
    sets = [sum(1 << j for j, x in enumerate(row) if x) for row in coef]
    evals = ctx.poly_evaluate_values_multi_dev(d_vals, log_n, _mont_list(points), sets)
    want = [[ol.poly_eval(c, t) if (m >> j) & 1 else 0 for j, t in enumerate(points)] for c, m in zip(coeffs, sets)]
    assert [ol.fr_ints(row) for row in evals] == want, what
    if n < 32:
        ints = [ol.fr_ints(v) for v in vals]
        assert ol.fr_ints(got) == kv.quotient_values(ints, log_n, points, coef), what


# ------------------------------------------------------------------------------------------------ the operator and the evaluations alone
@pytest.mark.parametrize("log_n", LOG_SIZES)
def test_operator_and_evaluations_against_the_oracle(ctx, log_n):
    n = 1 << log_n
    most = 64 if log_n <= 12 else 40
    vals, coeffs, d_vals, _ = _data(log_n, most)
    d_out = _dev(np.zeros((n, 4), dtype=np.uint64))
    # npoints 1, 2, 3 (of 4), 5 (of 8) and 8: every instantiation, exactly filled and padded; more than 32 polynomials: two launches of the sums
    for count, p in [(1, 1), (5, 2), (5, 3), (3, 5), (5, 8), (1, 8), (most, 1), (most, 8 if log_n <= 12 else 3)]:
        points = _points(n, p, seed=count)                                            # 1, r - 1, omega^3, omega^(N-1) on the domain; 0, 42, random off it
        coef = _coef(count, p, 7 * count + p, zero_row=1 if count > 1 else None, zero_col=1 if p > 1 else None)
        if count >= 5:
            coef[4] = [R_MOD - 1] * p
        _check_operator(ctx, log_n, vals[:count], coeffs[:count], d_vals[:count], d_out, points, coef, (log_n, count, p))
    for a, d in zip(vals, d_vals):
        assert np.array_equal(_host(d), a)                                            # the inputs are what they were


def test_directed_points_on_the_domain(ctx):
    """k at both ends, on both sides of the seam between the two tiles, two points in one lane's eight elements (x and x + 256), all eight
    points on the domain, the same point twice (legal for the operator alone)"""
    log_n, n = 12, 1 << 12
    vals, coeffs, d_vals, _ = _data(log_n, 6)
    d_out = _dev(np.zeros((n, 4), dtype=np.uint64))
    w = lambda k: _omega_pow(log_n, k)
    for ks in ([0], [TILE - 1], [TILE], [n - 1], [TILE - 1, TILE], [5, 5 + 256], [0, TILE - 1, TILE, n - 1, 5, 5 + 256, 5 + 7 * 256, 1],
               [3 * 256 + 77, None, 77], [9, 9]):
        points = [w(k) if k is not None else TAU for k in ks]
        coef = _coef(6, len(points), 31 + len(ks) + ks[0])
        coef[0] = [7] * len(points)                                                   # no empty column
        _check_operator(ctx, log_n, vals, coeffs, d_vals, d_out, points, coef, ks)


def test_extreme_values(ctx):
    log_n, n = 11, 1 << 11
    _key(ctx, log_n)
    top = np.tile(ol.fr_mont(R_MOD - 1), (n, 1))
    zero = np.zeros((n, 4), dtype=np.uint64)
    d_top, d_zero, d_out = _dev(top), _dev(zero), _dev(_rand_fr(n, 1))
    points = _points(n, 8)
    # 64 x 8 with every value and every coefficient r - 1 (the accumulators' bound); the polynomial is the constant r - 1: the quotient is zero
    ctx.poly_quotient_multi_values_dev([d_top] * 64, log_n, _mont_list(points), _mont_matrix([[R_MOD - 1] * 8] * 64), d_out)
    assert not _host(d_out).any()
    evals = ctx.poly_evaluate_values_multi_dev([d_top] * 64, log_n, _mont_list(points), [255] * 64)
    assert all(ol.fr_ints(row) == [R_MOD - 1] * 8 for row in evals)
    # r - 1 at every position but one: not a constant, every product at its largest
    spike = top.copy()
    spike[n - 1] = ol.fr_mont(1)
    c_spike = ol.ntt(spike, log_n, inverse=True)
    coef = [[R_MOD - 1] * 8 for _ in range(64)]
    ctx.poly_quotient_multi_values_dev([_dev(spike)] * 64, log_n, _mont_list(points), _mont_matrix(coef), d_out)
    assert np.array_equal(_host(d_out), _values_of(_quotient_ref([c_spike], points, [[64 * (R_MOD - 1) % R_MOD] * 8]), log_n))
    ctx.poly_quotient_multi_values_dev([d_zero], log_n, _mont_list(points[:3]), _mont_matrix([[5, 6, 7]]), d_out)
    assert not _host(d_out).any()
    # constants: h = 0, W and W' are infinity, and the verifier takes it
    import plonkit_amd as pa
    const = np.tile(ol.fr_mont(7), (n, 1))
    evals, u, proof = ctx.kzg_open_multi_values_dev([_dev(const)] * 2, log_n, _mont_list([9, 1]), [3, 2], ol.fr_mont(GAMMA), ol.fr_mont(5))
    assert not proof.any() and ol.fr_ints(evals[0]) == [7, 7] and ol.fr_ints(evals[1]) == [0, 7]
    assert pa.kzg_verify_multi(np.stack([_g(7)] * 2), _mont_list([9, 1]), [3, 2], evals, ol.fr_mont(GAMMA), u, proof, pa.crs42_g2_bytes()) is True
    # f_1 = f_2 with equal sets and gamma = r - 1: G_j = 0, W = infinity, and W' is what the coefficient route says
    f = _rand_fr(n, 2)
    d_f, d_c = _dev(f), _dev(ol.ntt(f, log_n, inverse=True))
    pts, sets, minus_one = _mont_list([TAU, R_MOD - 1, 0]), [7, 7], ol.fr_mont(R_MOD - 1)
    evals, u, proof = ctx.kzg_open_multi_values_dev([d_f, d_f], log_n, pts, sets, minus_one, ol.fr_mont(U_RANDOM))
    ev_c, u_c, proof_c = ctx.kzg_open_multi_dev([d_c, d_c], n, pts, sets, minus_one, ol.fr_mont(U_RANDOM))
    assert not proof[0].any() and proof.tobytes() == proof_c.tobytes() and evals.tobytes() == ev_c.tobytes()


# ------------------------------------------------------------------------------------------------ openings
def _check_opening(ctx, log_n, coeffs, d_coeffs, d_vals, points, sets, u, what, gamma=GAMMA):
    import plonkit_amd as pa
    n = 1 << log_n
    calls = []

    def challenge(w):
        calls.append(w.copy())
        return ol.fr_mont(u)

    pts, g = _mont_list(points), ol.fr_mont(gamma)
    evals, u_out, proof = ctx.kzg_open_multi_values_dev(d_vals, log_n, pts, sets, g, challenge)
    assert len(calls) == 1 and np.array_equal(calls[0], proof[0]), what               # once, with W
    assert np.array_equal(u_out, ol.fr_mont(u)), what
    want, h, q2 = _model_opening(coeffs, points, sets, gamma, u)                      # the oracle, in coefficients
    assert [ol.fr_ints(row) for row in evals] == want, what
    assert np.array_equal(proof[0], _g(ol.poly_eval(h, TAU))), what                   # the trapdoor
    assert np.array_equal(proof[1], _g(ol.poly_eval(q2, TAU))), what
    ev_c, u_c, proof_c = ctx.kzg_open_multi_dev(d_coeffs, n, pts, sets, g, ol.fr_mont(u))          # the coefficient route, byte for byte
    assert evals.tobytes() == ev_c.tobytes() and u_out.tobytes() == u_c.tobytes() and proof.tobytes() == proof_c.tobytes(), what
    cms = np.stack([_g(ol.poly_eval(c, TAU)) for c in coeffs])
    g2 = pa.crs42_g2_bytes()
    assert pa.kzg_verify_multi(cms, pts, sets, evals, g, u_out, proof, g2) is True, what
    i = len(coeffs) - 1
    j = km.members(sets[i], len(points))[0]
    if all(u != points[l] for l in range(len(points)) if l != j):       # (tests/test_kzg_multi_cases_host.py says why)
        bad = evals.copy()
        bad[i, j] = ol.fr_mont(want[i][j] + 1)
        assert pa.kzg_verify_multi(cms, pts, sets, bad, g, u_out, proof, g2) is False, what
    return evals, proof


@pytest.mark.parametrize("log_n", LOG_SIZES)
def test_openings_by_mask_family(ctx, log_n):
    n = 1 << log_n
    _key(ctx, log_n)
    vals, coeffs, d_vals, d_coeffs = _data(log_n, 32)
    pts8 = _points(n, 8)
    on = [t for t in pts8 if kv.on_domain(t, log_n)]
    assert len(on) >= 2 and TAU in pts8 and 0 in pts8
    cases = [("one at one", 1, [on[-1]], [1], U_RANDOM),                               # the point on the domain
             ("one at one", 1, [TAU], [1], U_RANDOM),
             ("plonk-like", 3, pts8[:3], km.plonk_like_masks(3), U_RANDOM),
             ("plonk-like", 3, [pts8[4], pts8[1], pts8[0]], km.plonk_like_masks(3), TAU),
             ("random", 32, pts8, km.random_masks(32, 8, 11), U_RANDOM)]
    for name, m, points, sets, u in cases:
        _check_opening(ctx, log_n, coeffs[:m], d_coeffs[:m], d_vals[:m], points, sets, u, (log_n, name))
    for a, d in zip(vals, d_vals):
        assert np.array_equal(_host(d), a)


def test_directed_challenges(ctx):
    """u = 0, 1 (omega^0), omega^5, a point of the opening off the domain and one on it, a position in the second tile"""
    log_n = 12
    _key(ctx, log_n)
    vals, coeffs, d_vals, d_coeffs = _data(log_n, 3)
    on = _omega_pow(log_n, TILE + 9)
    points, sets = [9, on, TAU], [3, 5, 6]
    for u in (0, 1, _omega_pow(log_n, 5), 9, on, _omega_pow(log_n, (1 << log_n) - 1)):
        _check_opening(ctx, log_n, coeffs, d_coeffs, d_vals, points, sets, u, ("u", u))


@pytest.mark.parametrize("m", [1, 2, 8])
def test_one_point_agrees_with_the_single_point_opening_from_values(ctx, m):
    log_n, n = 12, 1 << 12
    _key(ctx, log_n)
    vals, coeffs, d_vals, _ = _data(log_n, m)
    for z in (0, 5, TAU, R_MOD - 1, _omega_pow(log_n, 3)):                            # r - 1 = omega^(N/2) and omega^3 lie on the domain
        ev1, pi = ctx.kzg_open_dev(d_vals, n, ol.fr_mont(z), v=ol.fr_mont(GAMMA) if m > 1 else None, values=True)
        evals, u, proof = ctx.kzg_open_multi_values_dev(d_vals, log_n, _mont_list([z]), [1] * m, ol.fr_mont(GAMMA), ol.fr_mont(U_RANDOM))
        assert proof[0].tobytes() == pi.tobytes(), (m, z)
        assert np.array_equal(evals[:, 0], ev1), (m, z)
        if m == 1:
            assert np.array_equal(proof[1], proof[0]), z                              # L = (x - u) h


def test_refusals_and_the_context_after_them(ctx):
    import plonkit_amd as pa
    log_n, n = 8, 1 << 8
    _key(ctx, log_n)
    d = [_dev(_rand_fr(n, 40 + i)) for i in range(3)]
    d_out = _dev(np.zeros((n, 4), dtype=np.uint64))
    pts, gamma, u = _mont_list([9, 1, TAU]), ol.fr_mont(GAMMA), ol.fr_mont(77)
    sets = [3, 5, 6]
    calls = []

    def counted(w):
        calls.append(1)
        return u

    def refused(code, words, f, *a, **kw):
        with pytest.raises(pa.PlkError) as e:
            f(*a, **kw)
        assert e.value.code == code and words in str(e.value), e.value

    good = ctx.kzg_open_multi_values_dev(d, log_n, pts, sets, gamma, u)

    def still_works():
        again = ctx.kzg_open_multi_values_dev(d, log_n, pts, sets, gamma, u)
        assert all(np.array_equal(a, b) for a, b in zip(again, good))

    opening = ctx.kzg_open_multi_values_dev
    ctx.srs_lagrange_clear()                                                           # no Lagrange-form key
    refused(ERR_SRS, SIZE_WORDS, opening, d, log_n, pts, sets, gamma, counted)
    ctx.srs_lagrange_from_powers(log_n - 1)                                            # one of another size
    refused(ERR_SRS, SIZE_WORDS, opening, d, log_n, pts, sets, gamma, counted)
    ctx.poly_quotient_multi_values_dev(d, log_n, pts, _mont_matrix([[1, 2, 3]] * 3), d_out)        # the operator and the evaluations need no key
    ctx.poly_evaluate_values_multi_dev(d, log_n, pts, sets)
    ctx.srs_lagrange_from_powers(log_n)
    still_works()
    for bad_log in (0, 29):
        refused(ERR_ARG, "plk_kzg_open_multi_values_dev: bad argument", opening, d, bad_log, pts, sets, gamma, counted)
        refused(ERR_ARG, "plk_poly_quotient_multi_values_dev: bad argument", ctx.poly_quotient_multi_values_dev, d, bad_log, pts, _mont_matrix([[1, 2, 3]] * 3), d_out)
        refused(ERR_ARG, "plk_poly_evaluate_values_multi_dev: bad argument", ctx.poly_evaluate_values_multi_dev, d, bad_log, pts, sets)
    # km_common's and km_check_sets's words, with this call's name in front
    refused(ERR_ARG, "plk_kzg_open_multi_values_dev: two of the points are equal", opening, d, log_n, _mont_list([9, 1, 9]), sets, gamma, counted)
    refused(ERR_ARG, "empty set", opening, d, log_n, pts, [3, 0, 6], gamma, counted)
    refused(ERR_ARG, "does not exist", opening, d, log_n, pts, [3, 5, 14], gamma, counted)
    refused(ERR_ARG, "belongs to no set", opening, d, log_n, pts, [1, 1, 2], gamma, counted)
    refused(ERR_ARG, "not below r", opening, d, log_n, pts, sets, ol.int_to_limbs(R_MOD), counted)
    refused(ERR_ARG, "not below r", opening, d, log_n, np.stack([ol.int_to_limbs(R_MOD), pts[1], pts[2]]), sets, gamma, counted)
    refused(ERR_ARG, "bad argument", opening, [d[0]] * 33, log_n, _mont_list([9]), [1] * 33, gamma, counted)
    refused(ERR_ARG, "bad argument", opening, [0, d[1], d[2]], log_n, pts, sets, gamma, counted)
    refused(ERR_ARG, "16-byte aligned", opening, [d[0].data_ptr() + 8, d[1], d[2]], log_n, pts, sets, gamma, counted)
    refused(ERR_ARG, "does not exist", ctx.poly_evaluate_values_multi_dev, d, log_n, pts, [3, 5, 14])
    refused(ERR_ARG, "the output overlaps polynomial 1", ctx.poly_quotient_multi_values_dev, [d_out, d[0]], log_n, pts[:1], _mont_matrix([[1], [1]]), d[0])
    refused(ERR_ARG, "bad argument", ctx.poly_quotient_multi_values_dev, [d[0]] * 65, log_n, pts[:1], _mont_matrix([[1]] * 65), d_out)
    still_works()
    ctx.msm_enqueue_dev(d[0], n)                                                       # a commitment in flight
    try:
        refused(ERR_ARG, "a commitment is still in flight on this context", opening, d, log_n, pts, sets, gamma, counted)
        refused(ERR_ARG, "a commitment is still in flight on this context", ctx.poly_quotient_multi_values_dev, d, log_n, pts, _mont_matrix([[1, 2, 3]] * 3), d_out)
        refused(ERR_ARG, "a commitment is still in flight on this context", ctx.poly_evaluate_values_multi_dev, d, log_n, pts, sets)
    finally:
        ctx.msm_finish()
    assert calls == []                                                                 # no call that failed earlier reached the callback
    still_works()
    refused(ERR_IO, "plk_kzg_open_multi_values_dev: the challenge callback returned -7", opening, d, log_n, pts, sets, gamma, lambda w: -7)
    still_works()
    evals, u_out, proof = opening(d, log_n, pts, sets, gamma, counted)
    assert calls == [1] and np.array_equal(u_out, u) and np.array_equal(proof, good[2])
    refused(ERR_ARG, "not below r", opening, d, log_n, pts, sets, gamma, lambda w: ol.int_to_limbs(R_MOD))       # u >= r
    still_works()
    with pytest.raises(ZeroDivisionError):                                            # an exception of the callable comes back as itself
        opening(d, log_n, pts, sets, gamma, lambda w: 1 // 0)
    with pytest.raises(pa.PlkError):
        ctx.kzg_open_multi_last_ms()                                                   # nothing was timed
    ctx.set_kernel_timing(True)
    try:
        still_works()
        ms = ctx.kzg_open_multi_last_ms()                                              # the values route reports through the same four slots
        assert len(ms) == 4 and all(x > 0 for x in ms)
    finally:
        ctx.set_kernel_timing(False)
