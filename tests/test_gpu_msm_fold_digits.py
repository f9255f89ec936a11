"""Commitments through the two additions whose reductions fold their low Montgomery digits (field29_dev.h, "THE FOLD"; ec29_dev.h:
xyzzw_add_mixed_nflag in msm_accumulate's plain kernel, xyzzw_add_pairs in the 16-lane msm_task_reduce), over a tau = 42 key that holds no
point at infinity, every result bit-exact against the trapdoor value (one host scalar multiplication each).

Lengths: one term more than MSM_OWNED_MAX of msm_plan.h - the smallest length msm_plan_pass gives the plain kernel, odd - with four scalar
sets: uniform, a witness-like mix (half zeros, a quarter 16-bit values), all ones and all r - 1 (one hot bucket per window and the cold
P = +-Q path at every bucket boundary); and, at the same length, the smallest population at which a single bucket's task spans two slices:
16385 entries in one bucket (tests/gen/msm_bucket_cases.py: slices_one_bucket_16385).
Call styles: alone, as a batch of two, and as a batch of three - the batch of three is what launches the 16-lane reduction (asserted through
msm_last_shape).  Before a point is looked at the accumulation must report the plain instantiation without the point-at-infinity test."""
import os
import re

import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD
from tests.gen import msm_bucket_cases as gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTS = ("uniform", "witness_like", "ones", "minus_one")
SLICES = "slices_one_bucket_%d" % (gen.CHUNK + 1)
REDUCE_LANES = {1: 4, 2: 32, 3: 16}


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
        return _rand_fr(N, 31)
    if dist == "ones":
        return np.tile(ol.fr_mont(1), (N, 1))
    if dist == "minus_one":
        return np.tile(ol.fr_mont(R_MOD - 1), (N, 1))
    assert dist == "witness_like"                    # 50 % zero, 25 % repeated values below 2^16, 25 % uniform
    rng = np.random.default_rng(33)
    s = _rand_fr(N, 32)
    sel = rng.integers(0, 4, size=N)
    s[sel < 2] = 0
    idx = np.nonzero(sel == 2)[0]
    s[idx] = ol.fr_vec(list(range(1 << 16)))[rng.integers(0, 1 << 16, size=idx.shape[0])]
    return s


def _slices_case():
    """(scalars in Montgomery form, expected scalar) of the one-bucket case whose task spans two slices, in the plain build"""
    (case, k), = [(c, k) for c, k, b in gen.matrix() if c.name == SLICES and b == "plain"]
    assert case.n("plain") == N
    term_list = gen.terms(case, "plain", k)
    assert max(max(b) for b in gen.populations(term_list, "plain").values()) == gen.CHUNK + 1
    s = np.zeros((N, 4), dtype=np.uint64)
    by_value = {}
    for p, v in term_list:
        by_value.setdefault(v, []).append(p)
    for v, pos in by_value.items():
        s[np.array(pos, dtype=np.int64)] = ol.fr_mont(v)
    return s, gen.expected_scalar(term_list, N)


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    c.srs_generate(N, 0, 42)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """{name: (scalars, f(42) * G)}, computed once and left unchanged"""
    out = {}
    for d in DISTS:
        s = scalars(d)
        out[d] = (s, ol.g1_mul(ol.g1_generator(), ol.poly_eval(s, 42)))
    s, k = _slices_case()
    out[SLICES] = (s, ol.g1_mul(ol.g1_generator(), k))
    return out


def _plain_kernel_ran(ctx, batch):
    shape = ctx.msm_last_shape()
    assert shape["path"] == "ordinary" and shape["accumulate_variant"] == 0 and shape["bucket_sets"] == 1 and shape["batch"] == batch, shape
    assert shape["reduce_lanes"] == REDUCE_LANES[batch], shape
    assert ctx.msm_last_no_inf() is True


def test_the_length_is_the_first_past_the_owned_build():
    assert N == (1 << 16) + 1 and N == gen.BUILDS["plain"]["n"]


@pytest.mark.parametrize("name", DISTS + (SLICES,))
def test_one_commitment_against_the_trapdoor(ctx, cases, name):
    s, want = cases[name]
    got = ctx.msm(s)
    _plain_kernel_ran(ctx, 1)
    assert np.array_equal(np.asarray(got), want)


@pytest.mark.parametrize("group", [("uniform", "minus_one"), ("witness_like", SLICES), ("ones", SLICES, "uniform"), ("minus_one", "witness_like", "ones")],
                         ids=lambda g: "batch%d_%s" % (len(g), g[0]))
def test_a_batch_against_the_trapdoor(ctx, cases, group):
    """a batch of two reduces with 32 lanes a task, a batch of three with 16: msm_task_reduce<6, 4, true>, whose addition is xyzzw_add_pairs"""
    import torch
    dev = [torch.from_numpy(np.array(cases[d][0], copy=True).view(np.int64)).to("cuda:0") for d in group]
    torch.cuda.synchronize()
    got = list(ctx.msm_batch_dev(dev, N))
    _plain_kernel_ran(ctx, len(group))
    for d, g in zip(group, got):
        assert np.array_equal(np.asarray(g), cases[d][1]), d
