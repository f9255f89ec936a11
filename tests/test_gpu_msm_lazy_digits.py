"""Commitments through the two additions that take their products with lazy Montgomery digits (ec29_dev.h: xyzzw_add_mixed_flag in
msm_accumulate's plain kernel, xyzzw_add_pairs in the 16-lane msm_task_reduce a stream launches; field29_dev.h: the *_lz forms), at the
smallest length that takes the plain kernel: 2^16 + 256 terms over a tau = 42 key of that size.

Three scalar sets - uniform, all r - 1 (one hot bucket per window and the cold P = +-Q path at every bucket boundary), a witness-like
mix (half zeros, a quarter 16-bit values) - each against the trapdoor value (one host scalar multiplication), the uniform set against
the CPU oracle's MSM as well; then the same three as a stream with three in flight, byte for byte the one-at-a-time results.  The
accumulation must report the instantiation without the point-at-infinity test; a key with one point at infinity takes the unchanged
kernel and still gives the right point."""
import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD

pytestmark = pytest.mark.gpu

N = (1 << 16) + 256
DISTS = ("uniform", "minus_one", "witness_like")
INF_AT = 40000


def _rand_fr(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)             # < 2^252 < r: valid Montgomery residues
    return a


def scalars(dist):
    if dist == "uniform":
        return _rand_fr(N, 11)
    if dist == "minus_one":
        return np.tile(ol.fr_mont(R_MOD - 1), (N, 1))
    assert dist == "witness_like"                    # 50 % zero, 25 % repeated values below 2^16, 25 % uniform
    rng = np.random.default_rng(13)
    s = _rand_fr(N, 12)
    sel = rng.integers(0, 4, size=N)
    s[sel < 2] = 0
    idx = np.nonzero(sel == 2)[0]
    s[idx] = ol.fr_vec(list(range(1 << 16)))[rng.integers(0, 1 << 16, size=idx.shape[0])]
    return s


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    c.srs_generate(N, 0, 42)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """{distribution: (scalars, f(42), f(42) * G)}, computed once"""
    out = {}
    for d in DISTS:
        s = scalars(d)
        k = ol.poly_eval(s, 42)
        out[d] = (s, k, ol.g1_mul(ol.g1_generator(), k))
    return out


@pytest.fixture(scope="module")
def singles(ctx, cases):
    """the one-at-a-time commitments (the reduction by quads), each with the kernel the accumulation reported"""
    out = {}
    for d in DISTS:
        got = ctx.msm(cases[d][0])
        shape = ctx.msm_last_shape()
        out[d] = (np.asarray(got), shape, ctx.msm_last_no_inf())
    return out


@pytest.mark.parametrize("dist", DISTS)
def test_one_commitment_against_the_trapdoor(cases, singles, dist):
    got, shape, no_inf = singles[dist]
    assert shape["path"] == "ordinary" and shape["accumulate_variant"] == 0 and shape["bucket_sets"] == 1 and shape["window_bits"] == 17, shape
    assert no_inf is True
    assert np.array_equal(got, cases[dist][2])


def test_uniform_scalars_against_the_oracle_msm(ctx, cases, singles):
    key = ctx.srs_download(0, N)
    assert np.array_equal(singles["uniform"][0], ol.msm(key, cases["uniform"][0]))


def test_stream_of_three_in_flight_is_byte_identical(ctx, cases, singles):
    """commit_stream keeps three commitments in flight: the second and third are reduced by msm_task_reduce<6, 4, true>"""
    import torch
    from plonkit_amd.sharded import ShardedMsm
    dev = torch.device("cuda:0")
    order = list(DISTS) + list(DISTS)               # six commitments: the stream stays full while the first three finish
    vecs = {d: torch.from_numpy(cases[d][0].view(np.int64)).to(dev) for d in DISTS}
    torch.cuda.synchronize()
    got, lanes = [], []
    for out in ShardedMsm(ctx, None, dev).commit_stream((vecs[d] for d in order), N, depth=3):
        got.append(np.asarray(out))
        lanes.append(ctx.msm_last_shape()["reduce_lanes"])
        assert ctx.msm_last_no_inf() is True
    assert len(got) == 6
    assert 16 in lanes, lanes                        # the work-priced reduction ran
    for d, g in zip(order, got):
        assert g.tobytes() == singles[d][0].tobytes(), d


def test_key_with_a_point_at_infinity_takes_the_unchanged_kernel(cases):
    import plonkit_amd as pa
    c = pa.Context(0)
    try:
        c.srs_generate(N, 0, 42)
        key = c.srs_download(0, N)
        key[INF_AT] = 0
        c.srs_upload(key)
        s, k, _ = cases["uniform"]
        got = c.msm(s)
        shape = c.msm_last_shape()
        assert shape["path"] == "ordinary" and shape["accumulate_variant"] == 0, shape
        assert c.msm_last_no_inf() is False
        k = (k - ol.fr_ints(np.ascontiguousarray(s[INF_AT:INF_AT + 1]))[0] * pow(42, INF_AT, R_MOD)) % R_MOD
        assert np.array_equal(got, ol.g1_mul(ol.g1_generator(), k))
    finally:
        c.close()
