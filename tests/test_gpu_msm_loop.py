"""The flat loop of msm_accumulate's plain kernel (more than 2^16 terms: equal pieces per lane) and the addition it runs
(ec29_dev.h: xyzzw_add_mixed_flag — addends folded into the products, a lane flag instead of the is_inf(acc) test, no is_inf(q) test
when the key's table holds no point at infinity).  Commitments of 2^16 + 1 and 2^17 terms over a 2^17-point tau = 42 key against the
trapdoor value (one host scalar multiplication each): uniform scalars, all-ones and all-(r - 1) (one hot bucket per window, every
bucket boundary), equal and opposite points meeting in a bucket (duplicate and negated bases under equal scalars: the special path,
and an accumulator that returns to the identity and starts again), a witness-like mix with zeros, and a key that holds the point at
infinity, which must take the kept kernel.  Then the flag that selects the kernel: it follows the key through every change of it.

The reference of a key whose points were replaced: base j = c_j * G with c_j = 42^j, +-42^k or 0, so the commitment is
(poly_eval(s, 42) + sum over the replaced j of s_j (c_j - 42^j)) * G."""
import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD

pytestmark = pytest.mark.gpu

KEY_N = 1 << 17
SIZES = (KEY_N // 2 + 1, KEY_N)                     # 2^16 + 1: the first length that takes the plain kernel; 2^17: the whole key
DUP, RUN = 7, 3000                                  # bases [0, RUN) = B_7, [RUN, 2 RUN) = -B_7
INF_AT = (100, 50000, KEY_N // 2)                   # the key with points at infinity (the last one: the last base of the shorter commitment)


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys(ctx):
    """the clean key (as generated on the GPU), the key with duplicate and negated bases, the key with points at infinity, and for
    the latter two {index: c_j}"""
    ctx.srs_generate(KEY_N, 0, 42)
    clean = ctx.srs_download(0, KEY_N)
    dup = clean.copy()
    dup[:RUN] = clean[DUP]
    dup[RUN:2 * RUN] = ol.g1_neg(clean[DUP])
    c = pow(42, DUP, R_MOD)
    dup_c = {j: (c if j < RUN else R_MOD - c) for j in range(2 * RUN)}
    inf = clean.copy()
    for j in INF_AT:
        inf[j] = 0
    return dict(clean=(clean, {}), dup=(dup, dup_c), inf=(inf, {j: 0 for j in INF_AT}))


def _rand_fr(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)             # < 2^252 < r: valid Montgomery residues
    return a


_SMALL = []


def scalars(dist, n, seed):
    if dist == "uniform":
        return _rand_fr(n, seed)
    if dist in ("ones", "minus_one"):
        return np.tile(ol.fr_mont(1 if dist == "ones" else R_MOD - 1), (n, 1))
    if dist == "meet":                               # equal scalars over the duplicate and negated bases, uniform elsewhere
        s = _rand_fr(n, seed)
        s[:2 * RUN] = s[0]
        s[RUN // 2:RUN] = s[1]                       # a second bucket in which P + P happens first
        return s
    assert dist == "witness_like"                    # 50 % zero, 25 % below 2^16, 25 % uniform
    if not _SMALL:
        _SMALL.append(ol.fr_vec(list(range(1 << 16))))
    rng = np.random.default_rng(seed + 1)
    s = _rand_fr(n, seed)
    sel = rng.integers(0, 4, size=n)
    s[sel < 2] = 0
    idx = np.nonzero(sel == 2)[0]
    s[idx] = _SMALL[0][rng.integers(0, 1 << 16, size=idx.shape[0])]
    return s


def expected(s, replaced):
    k = ol.poly_eval(s, 42)
    if replaced:
        idx = [j for j in sorted(replaced) if j < s.shape[0]]
        vals = ol.fr_ints(np.ascontiguousarray(s[idx]))
        k = (k + sum(v * (replaced[j] - pow(42, j, R_MOD)) for j, v in zip(idx, vals))) % R_MOD
    return ol.g1_mul(ol.g1_generator(), k)


def commit(ctx, s, replaced, no_inf):
    got = ctx.msm(s)
    shape = ctx.msm_last_shape()
    assert shape["path"] == "ordinary" and shape["accumulate_variant"] == 0 and shape["bucket_sets"] == 1, shape
    assert ctx.msm_last_no_inf() is no_inf
    assert np.array_equal(got, expected(s, replaced))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dist", ["uniform", "ones", "minus_one", "witness_like"])
def test_plain_kernel_on_a_clean_key(ctx, keys, dist, n):
    ctx.srs_upload(keys["clean"][0])
    commit(ctx, scalars(dist, n, n + len(dist)), {}, True)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dist", ["meet", "ones", "uniform"])
def test_equal_and_opposite_points_in_a_bucket(ctx, keys, dist, n):
    """3000 x P and 3000 x (-P) under one scalar: P + P, then the sum walks back through P + (-P) = identity and starts again"""
    key, replaced = keys["dup"]
    ctx.srs_upload(key)
    commit(ctx, scalars(dist, n, 3 * n), replaced, True)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dist", ["uniform", "minus_one", "witness_like"])
def test_key_with_points_at_infinity_keeps_the_tested_kernel(ctx, keys, dist, n):
    key, replaced = keys["inf"]
    ctx.srs_upload(key)
    commit(ctx, scalars(dist, n, 5 * n), replaced, False)


def test_the_flag_follows_the_key(ctx, keys):
    """one context: clean -> with infinity -> clean (generated) -> with infinity -> clean (uploaded); a borrower of the key sees the
    lender's flag; a key whose ONLY point at infinity lies beyond the commitment still takes the kept kernel (the flag is the table's)"""
    import plonkit_amd as pa
    n = SIZES[0]
    s = scalars("uniform", n, 99)
    inf_key, inf_c = keys["inf"]
    ctx.srs_upload(keys["clean"][0])
    commit(ctx, s, {}, True)
    ctx.srs_upload(inf_key)
    commit(ctx, s, inf_c, False)
    ctx.srs_generate(KEY_N, 0, 42)
    commit(ctx, s, {}, True)
    late = keys["clean"][0].copy()
    late[KEY_N - 1] = 0
    ctx.srs_upload(late)
    commit(ctx, s, {KEY_N - 1: 0}, False)
    other = pa.Context(0)
    try:
        other.share_srs_from(ctx)
        commit(other, s, {KEY_N - 1: 0}, False)
    finally:
        other.close()
    ctx.srs_upload(keys["clean"][0])
    commit(ctx, s, {}, True)
    other = pa.Context(0)
    try:
        other.share_srs_from(ctx)
        commit(other, s, {}, True)
        other.srs_upload(inf_key)                    # a key of its own ends the loan
        commit(other, s, inf_c, False)
        commit(ctx, s, {}, True)
    finally:
        other.close()
