"""Commitments through the mixed addition that reduces the shared factor P^2 once (ec29_dev.h: xyzzw_add_mixed_nflag on field29_dev.h's
make_tw2_a / mul_tw2_2 / mul_tw2_mulw), which only msm_accumulate's plain kernel reaches: at the smallest length that msm_plan_pass gives
that kernel - one term more than MSM_OWNED_MAX of msm_plan.h, an odd length - over a tau = 42 key of that size, which holds no point at
infinity.

Four scalar sets - uniform, a witness-like mix (half zeros, a quarter 16-bit values), all ones and all r - 1 (the last two: one hot bucket
per window, the repeated-scalar tasks of the same kernel, and the cold P = +-Q path at every bucket boundary) - each against the trapdoor
value (one host scalar multiplication); then two of them as one batch of two.  The accumulation must report the plain instantiation without
the point-at-infinity test."""
import os
import re

import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTS = ("uniform", "witness_like", "ones", "minus_one")


def _owned_max():
    with open(os.path.join(ROOT, "plonkit_amd", "csrc", "msm_plan.h")) as f:
        m = re.search(r"MSM_OWNED_MAX = 1ull << (\d+);", f.read())
    assert m, "msm_plan.h no longer states MSM_OWNED_MAX as a power of two"
    return 1 << int(m.group(1))


N = _owned_max() + 1


def _rand_fr(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)             # < 2^252 < r: valid Montgomery residues
    return a


def scalars(dist):
    if dist == "uniform":
        return _rand_fr(N, 21)
    if dist == "ones":
        return np.tile(ol.fr_mont(1), (N, 1))
    if dist == "minus_one":
        return np.tile(ol.fr_mont(R_MOD - 1), (N, 1))
    assert dist == "witness_like"                    # 50 % zero, 25 % repeated values below 2^16, 25 % uniform
    rng = np.random.default_rng(23)
    s = _rand_fr(N, 22)
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
    """{distribution: (scalars, f(42) * G)}, computed once"""
    out = {}
    for d in DISTS:
        s = scalars(d)
        out[d] = (s, ol.g1_mul(ol.g1_generator(), ol.poly_eval(s, 42)))
    return out


def _plain_kernel_ran(ctx, batch):
    shape = ctx.msm_last_shape()
    assert shape["path"] == "ordinary" and shape["accumulate_variant"] == 0 and shape["bucket_sets"] == 1 and shape["batch"] == batch, shape
    assert ctx.msm_last_no_inf() is True


def test_the_length_is_the_first_past_the_owned_build():
    assert N == (1 << 16) + 1


@pytest.mark.parametrize("dist", DISTS)
def test_one_commitment_against_the_trapdoor(ctx, cases, dist):
    s, want = cases[dist]
    got = ctx.msm(s)
    _plain_kernel_ran(ctx, 1)
    assert np.array_equal(np.asarray(got), want)


def test_a_batch_of_two_against_the_trapdoor(ctx, cases):
    import torch
    pair = ("uniform", "minus_one")
    dev = [torch.from_numpy(cases[d][0].view(np.int64)).to("cuda:0") for d in pair]
    torch.cuda.synchronize()
    got = list(ctx.msm_batch_dev(dev, N))
    _plain_kernel_ran(ctx, 2)
    for d, g in zip(pair, got):
        assert np.array_equal(np.asarray(g), cases[d][1]), d
