"""-m gpu: many polynomials at several points with a proof of two points (kzg_multi.hip): the multi-point quotient kernels through
plk_poly_quotient_multi_dev, plk_kzg_open_multi_dev, and plk_kzg_verify_multi on what it returns.

Referees.  The quotient: the grouped formula sum_j D_{t_j}[sum_i coef_ij f_i] through the oracle's C routines (ol.vaxpy / ol.vscale /
ol.poly_div_linear), and below n = 32 the Python-integer model of tests/gen/kzg_multi_cases.py, whose host test holds the grouped formula
against interpolation and long division.  The openings: the trapdoor of the tau = 42 key — W = h(42) G and W' = Q(42) G with h and Q
from the oracle's coefficients (no division by 42 - t occurs, so t_j = 42 and u = 42 are ordinary cases) — ol.poly_eval for the
evaluations, plk_kzg_open_dev for one point.  Equality is bit for bit: exact arithmetic, no tolerance.
THE TILE is the scan engine's 2048 coefficients (8 per lane, 256 lanes): the sizes below stand on both sides of one and of three."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD
from tests.gen import kzg_multi_cases as km

ERR_ARG, ERR_SRS, ERR_IO = 1, 3, 7
TAU = km.TAU
TILE = 2048
TOP = 0x30644e72e131a029
GAMMA = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80919 % R_MOD
G = ol.g1_generator()


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    c.srs_generate(1 << 16, 0, TAU)
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


def _g(k):
    return ol.g1_mul(G, k % R_MOD) if k % R_MOD else np.zeros(8, dtype=np.uint64)


def _mont_matrix(rows):
    return np.stack([np.stack([ol.fr_mont(x) for x in row]) for row in rows])


def _mont_list(xs):
    return np.stack([ol.fr_mont(x) for x in xs])


def _quotient_ref(polys, points, coef):
    """sum_j D_{t_j}[sum_i coef[i][j] f_i] by the oracle's C routines; polys are [n, 4] Montgomery arrays"""
    n = polys[0].shape[0]
    out = np.zeros((n, 4), dtype=np.uint64)
    for j, t in enumerate(points):
        g = np.zeros((n, 4), dtype=np.uint64)
        for f, row in zip(polys, coef):
            if row[j]:
                g = ol.vaxpy(g, row[j], f)
        out = ol.vadd(out, ol.poly_div_linear(g, t))
    return out


def _points(n, p, seed=0):
    """p distinct points: 0, 1, r - 1, omega^k of the size and 42 first (turned by the seed, so that one-point shapes meet more than 0), then random ones"""
    log_n = max(n - 1, 1).bit_length()
    w = km.omega(log_n)
    pool = []
    for t in (0, 1, R_MOD - 1, pow(w, 3, R_MOD), TAU, pow(w, (1 << log_n) - 1, R_MOD)):
        if t not in pool:
            pool.append(t)
    pool = pool[seed % 5:] + pool[:seed % 5]
    rng = np.random.default_rng(1000 + seed)
    while len(pool) < 8:
        t = int(rng.integers(2, 1 << 62)) * 0x9e3779b97f4a7c15 % R_MOD
        if t not in pool:
            pool.append(t)
    return pool[:p]


def _coef(count, p, seed, zero_row=None, zero_col=None):
    rng = np.random.default_rng(seed)
    rows = [[int(x) * 0x1234567890abcdef1234567 % R_MOD if rng.integers(0, 4) else 0 for x in rng.integers(1, 1 << 62, size=p)] for _ in range(count)]
    if zero_row is not None:
        rows[zero_row] = [0] * p
    if zero_col is not None:
        for row in rows:
            row[zero_col] = 0
    return rows


# ------------------------------------------------------------------------------------------------ the kernels on their own
SIZES = (1, 2, 7, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, (1 << 16) + 3)


@pytest.mark.parametrize("n", SIZES)
def test_quotient_kernels_against_the_grouped_formula(ctx, n):
    polys64 = [_rand_fr(n, 64 * n + i) for i in range(64)]
    polys64[3] = np.zeros((n, 4), dtype=np.uint64)                                    # a zero polynomial among the inputs
    polys64[4] = np.tile(ol.fr_mont(R_MOD - 1), (n, 1))                               # every coefficient r - 1
    polys64[7] = polys64[4]
    d64 = [_dev(a) for a in polys64]
    d_out = _dev(np.zeros((n, 4), dtype=np.uint64))
    # npoints 1, 2, 3 (of 4), 5 (of 8) and 8: every instantiation of the tile kernel, exactly filled and padded
    shapes = [(1, 1), (5, 2), (5, 3), (3, 5), (5, 8), (1, 8), (64, 1)] + ([(64, 8), (64, 3)] if n <= 3 * TILE + 5 else [])
    for count, p in shapes:
        points = _points(n, p, seed=count)
        coef = _coef(count, p, 7 * count + p, zero_row=1 if count > 1 else None, zero_col=1 if p > 1 else None)
        if count >= 5:
            coef[4] = [R_MOD - 1] * p                                                 # (r - 1) x (r - 1) at every point
        ctx.poly_quotient_multi_dev(d64[:count], n, _mont_list(points), _mont_matrix(coef), d_out)
        got = _host(d_out)
        assert np.array_equal(got, _quotient_ref(polys64[:count], points, coef)), (n, count, p)
        if n < 32:
            assert ol.fr_ints(got) == km.quotient_multi([ol.fr_ints(a) for a in polys64[:count]], points, coef), (n, count, p)
    for a, d in zip(polys64, d64):
        assert np.array_equal(_host(d), a)                                            # the inputs are what they were


def test_quotient_of_extreme_inputs(ctx):
    """all polynomials r - 1 with all coefficients r - 1 at 64 x 8 (the accumulators' bound), a zero polynomial alone, the same pointer twice"""
    n = TILE + 1
    top = np.tile(ol.fr_mont(R_MOD - 1), (n, 1))
    d_top, d_zero, d_out = _dev(top), _dev(np.zeros((n, 4), dtype=np.uint64)), _dev(_rand_fr(n, 1))
    points = _points(n, 8)
    coef = [[R_MOD - 1] * 8 for _ in range(64)]
    ctx.poly_quotient_multi_dev([d_top] * 64, n, _mont_list(points), _mont_matrix(coef), d_out)
    assert np.array_equal(_host(d_out), _quotient_ref([top], points, [[64 * (R_MOD - 1) % R_MOD] * 8]))
    ctx.poly_quotient_multi_dev([d_zero], n, _mont_list(points[:3]), _mont_matrix([[5, 6, 7]]), d_out)
    assert not _host(d_out).any()
    f = _rand_fr(n, 2)
    d_f = _dev(f)
    ctx.poly_quotient_multi_dev([d_f, d_f], n, _mont_list([TAU]), _mont_matrix([[3], [4]]), d_out)
    assert np.array_equal(_host(d_out), ol.poly_div_linear(ol.vscale(f, 7), TAU))


def test_quotient_refusals(ctx):
    import plonkit_amd as pa
    n = 100
    d, d_out = _dev(_rand_fr(n, 3)), _dev(np.zeros((n, 4), dtype=np.uint64))
    one = _mont_list([1])

    def refused(code, words, f, *a, **kw):
        with pytest.raises(pa.PlkError) as e:
            f(*a, **kw)
        assert e.value.code == code and words in str(e.value), e.value

    refused(ERR_ARG, "the output overlaps polynomial 1", ctx.poly_quotient_multi_dev, [d_out, d], n, one, _mont_matrix([[1], [1]]), d)
    refused(ERR_ARG, "bad argument", ctx.poly_quotient_multi_dev, [d] * 65, n, one, _mont_matrix([[1]] * 65), d_out)
    refused(ERR_ARG, "bad argument", ctx.poly_quotient_multi_dev, [d], n, _mont_list(range(9)), _mont_matrix([list(range(9))]), d_out)
    refused(ERR_ARG, "bad argument", ctx.poly_quotient_multi_dev, [0], n, one, _mont_matrix([[1]]), d_out)
    refused(ERR_ARG, "not below r", ctx.poly_quotient_multi_dev, [d], n, np.stack([ol.int_to_limbs(R_MOD)]), _mont_matrix([[1]]), d_out)
    refused(ERR_ARG, "16-byte aligned", ctx.poly_quotient_multi_dev, [d.data_ptr() + 8], n - 1, one, _mont_matrix([[1]]), d_out)
    ctx.poly_quotient_multi_dev([d], n, one, _mont_matrix([[1]]), d_out)               # and the context still works
    assert np.array_equal(_host(d_out), ol.poly_div_linear(_host(d), 1))


# ------------------------------------------------------------------------------------------------ openings
def _model_opening(polys, points, sets, gamma, u):
    """(evals as ints [m][p], h, Q) with h and Q from the oracle's coefficients: the grouped formula, twice"""
    h = _quotient_ref(polys, points, km.matrix(points, sets, gamma))
    c, z_t = km.c_values(points, sets, gamma, u)
    q2 = _quotient_ref(list(polys) + [h], [u], [[x] for x in c] + [[(-z_t) % R_MOD]])
    evals = [[ol.poly_eval(f, t) if (m >> j) & 1 else 0 for j, t in enumerate(points)] for f, m in zip(polys, sets)]
    return evals, h, q2


def _check_opening(ctx, polys, d_polys, n, points, sets, u, what):
    import plonkit_amd as pa
    calls = []

    def challenge(w):
        calls.append(w.copy())
        return ol.fr_mont(u)

    evals, u_out, proof = ctx.kzg_open_multi_dev(d_polys, n, _mont_list(points), sets, ol.fr_mont(GAMMA), challenge)
    assert len(calls) == 1 and np.array_equal(calls[0], proof[0]), what               # once, with W
    assert np.array_equal(u_out, ol.fr_mont(u)), what
    want, h, q2 = _model_opening(polys, points, sets, GAMMA, u)
    assert [ol.fr_ints(row) for row in evals] == want, what
    assert np.array_equal(proof[0], _g(ol.poly_eval(h, TAU))), what
    assert np.array_equal(proof[1], _g(ol.poly_eval(q2, TAU))), what
    cms = np.stack([_g(ol.poly_eval(f, TAU)) for f in polys])
    g2 = pa.crs42_g2_bytes()
    assert pa.kzg_verify_multi(cms, _mont_list(points), sets, evals, ol.fr_mont(GAMMA), u_out, proof, g2) is True, what
    i = len(polys) - 1
    j = km.members(sets[i], len(points))[0]
    if all(u != points[l] for l in range(len(points)) if l != j):       # (tests/test_kzg_multi_cases_host.py says why)
        bad = evals.copy()
        bad[i, j] = ol.fr_mont(want[i][j] + 1)
        assert pa.kzg_verify_multi(cms, _mont_list(points), sets, bad, ol.fr_mont(GAMMA), u_out, proof, g2) is False, what
    return evals, proof


U_RANDOM = 0x1f2e3d4c5b6a79880706050403020100fedcba98765432100123456789abcdef % R_MOD


@pytest.mark.parametrize("n", [TILE + 1, 1 << 16])
def test_openings_by_mask_family(ctx, n):
    polys = [_rand_fr(n, 32 * (n % 1000) + i) for i in range(32)]
    polys[2] = np.zeros((n, 4), dtype=np.uint64)
    d_polys = [_dev(a) for a in polys]
    pts8 = _points(n, 8)                                                              # 0, 1, r - 1, a domain point, 42, ...
    assert TAU in pts8[:5] and 0 in pts8[:3]
    cases = [("singletons", 3, pts8[:3], km.singleton_masks(3, 3), U_RANDOM),
             ("all at all", 4, pts8[:5], km.all_masks(4, 5), U_RANDOM),               # t_j = 42 among the points
             ("plonk-like", 8, pts8[:3], km.plonk_like_masks(8), TAU),                # u = 42
             ("plonk-like", 8, [pts8[4], pts8[1], pts8[0]], km.plonk_like_masks(8), U_RANDOM),
             ("random", 32, pts8, km.random_masks(32, 8, 11), U_RANDOM)]
    for name, m, points, sets, u in cases:
        _check_opening(ctx, polys[:m], d_polys[:m], n, points, sets, u, (n, name))
    for a, d in zip(polys, d_polys):
        assert np.array_equal(_host(d), a)


@pytest.mark.parametrize("m", [1, 2, 8])
def test_one_point_agrees_with_the_single_point_opening(ctx, m):
    n = 3 * TILE + 5
    polys = [_rand_fr(n, 900 + i) for i in range(m)]
    d_polys = [_dev(a) for a in polys]
    for z in (0, 5, TAU, R_MOD - 1):
        ev1, pi = ctx.kzg_open_dev(d_polys, n, ol.fr_mont(z), v=ol.fr_mont(GAMMA) if m > 1 else None)
        evals, u, proof = ctx.kzg_open_multi_dev(d_polys, n, _mont_list([z]), [1] * m, ol.fr_mont(GAMMA), ol.fr_mont(U_RANDOM))
        assert proof[0].tobytes() == pi.tobytes(), (m, z)
        assert np.array_equal(evals[:, 0], ev1), (m, z)
        if m == 1:
            assert np.array_equal(proof[1], proof[0]), z                              # L = (x - u) h


def test_edges_of_the_opening(ctx):
    import plonkit_amd as pa
    n = TILE + 1
    polys = [_rand_fr(n, 70 + i) for i in range(3)]
    d_polys = [_dev(a) for a in polys]
    points, sets = [9, 0, TAU], [3, 5, 6]
    for u in (0, 9, TAU):                                                             # u = 0, u = t_0, u = 42
        _check_opening(ctx, polys, d_polys, n, points, sets, u, ("u", u))
    # n = 1: both quotients are empty
    evals, u, proof = ctx.kzg_open_multi_dev([d_polys[0]], 1, _mont_list([9]), [1], ol.fr_mont(GAMMA), ol.fr_mont(5))
    assert not proof.any() and np.array_equal(evals[0, 0], polys[0][0])
    # constants: infinity as W and W', and the verifier takes it
    const = np.zeros((n, 4), dtype=np.uint64)
    const[0] = ol.fr_mont(7)
    evals, u, proof = ctx.kzg_open_multi_dev([_dev(const)] * 2, n, _mont_list([9, 0]), [3, 2], ol.fr_mont(GAMMA), ol.fr_mont(5))
    assert not proof.any()
    assert pa.kzg_verify_multi(np.stack([_g(7)] * 2), _mont_list([9, 0]), [3, 2], evals, ol.fr_mont(GAMMA), u, proof, pa.crs42_g2_bytes()) is True


def test_refusals_of_the_opening_and_the_callback(ctx):
    import plonkit_amd as pa
    n = 300
    d = [_dev(_rand_fr(n, 40 + i)) for i in range(3)]
    pts, gamma, u = _mont_list([9, 0, TAU]), ol.fr_mont(GAMMA), ol.fr_mont(77)
    sets = [3, 5, 6]

    def refused(code, words, *a, **kw):
        with pytest.raises(pa.PlkError) as e:
            ctx.kzg_open_multi_dev(*a, **kw)
        assert e.value.code == code and words in str(e.value), e.value

    calls = []

    def counted(w):
        calls.append(1)
        return u

    refused(ERR_ARG, "two of the points are equal", d, n, _mont_list([9, 0, 9]), sets, gamma, counted)
    refused(ERR_ARG, "empty set", d, n, pts, [3, 0, 6], gamma, counted)
    refused(ERR_ARG, "does not exist", d, n, pts, [3, 5, 14], gamma, counted)
    refused(ERR_ARG, "belongs to no set", d, n, pts, [1, 1, 2], gamma, counted)
    refused(ERR_ARG, "not below r", d, n, pts, sets, ol.int_to_limbs(R_MOD), counted)
    refused(ERR_ARG, "not below r", d, n, np.stack([ol.int_to_limbs(R_MOD), pts[1], pts[2]]), sets, gamma, counted)
    refused(ERR_ARG, "bad argument", [d[0]] * 33, n, _mont_list([9]), [1] * 33, gamma, counted)
    refused(ERR_ARG, "bad argument", [0, d[1], d[2]], n, pts, sets, gamma, counted)
    refused(ERR_ARG, "16-byte aligned", [d[0].data_ptr() + 8, d[1], d[2]], n - 1, pts, sets, gamma, counted)
    refused(ERR_SRS, "no key resident, or the key is shorter than the polynomials", d, (1 << 16) + 1, pts, sets, gamma, counted)
    ctx.msm_enqueue_dev(d[0], n)                                                       # a commitment in flight
    try:
        refused(ERR_ARG, "a commitment is still in flight on this context", d, n, pts, sets, gamma, counted)
    finally:
        ctx.msm_finish()
    assert calls == []                                                                 # no call that failed earlier reached the callback
    refused(ERR_IO, "the challenge callback returned -7", d, n, pts, sets, gamma, lambda w: -7)
    evals, u_out, proof = ctx.kzg_open_multi_dev(d, n, pts, sets, gamma, counted)     # the next call succeeds
    assert calls == [1] and np.array_equal(u_out, u)
    refused(ERR_ARG, "not below r", d, n, pts, sets, gamma, lambda w: ol.int_to_limbs(R_MOD))     # u >= r
    again = ctx.kzg_open_multi_dev(d, n, pts, sets, gamma, u)                          # a fixed scalar; the context is still usable
    assert np.array_equal(again[2], proof) and np.array_equal(again[0], evals)
    with pytest.raises(ZeroDivisionError):                                            # an exception of the callable comes back as itself
        ctx.kzg_open_multi_dev(d, n, pts, sets, gamma, lambda w: 1 // 0)
    with pytest.raises(pa.PlkError):
        ctx.kzg_open_multi_last_ms()                                                   # nothing was timed
