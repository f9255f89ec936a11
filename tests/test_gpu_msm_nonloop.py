"""The kernels of a commitment around msm_accumulate, at the smallest lengths that reach the instantiations priced by work:
msm_recode_count / msm_recode_scatter (scalars leave Montgomery form on the 29-bit layer, digits from its limbs, canonical words handed
from the first pass to the second) and the 16-lane msm_task_reduce whose one addition is xyzzw_add_pairs.  Commitments over a
2^17-point tau = 42 key against the trapdoor value (one host scalar multiplication each):

  * 2^15 + 1 and 2^16 + 3 terms alone: just above the short path, the ordinary pipeline's recoding at its smallest (and, alone on the
    context, the untouched reduction by quads);
  * 2^16 + 3 and 2^17 terms three ways — a batch of three and a commitment enqueued while another is in flight (16 lanes per task: the
    changed reduction), and alone (quads) — over uniform scalars, all ones and all r - 1 (one hot bucket per window: msm_fold_hot's slot
    is read by the reduction), a witness-like mix (half zeros, a quarter 16-bit values) and a vector that is zero except for one term;
  * a batch of three DIFFERENT vectors: the canonical words of vector m lie at m * n of the hand-over buffer.

Context.msm_last_shape() must report the reduction each case is meant to reach."""
import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD

pytestmark = pytest.mark.gpu

KEY_N = 1 << 17
DISTS = ("uniform", "ones", "minus_one", "witness_like", "one_hot")


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    c.srs_generate(KEY_N, 0, 42)
    yield c
    c.close()


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
    if dist == "one_hot":
        s = np.zeros((n, 4), dtype=np.uint64)
        s[(seed * 7919) % n] = ol.fr_mont(R_MOD - 2 - seed)
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


_EXPECTED = {}


def expected(dist, n, seed):
    """(scalars, trapdoor value), computed once per (distribution, length, seed)"""
    key = (dist, n, seed)
    if key not in _EXPECTED:
        s = scalars(dist, n, seed)
        _EXPECTED[key] = (s, ol.g1_mul(ol.g1_generator(), ol.poly_eval(s, 42)))
    return _EXPECTED[key]


def _dev(s):
    import torch
    t = torch.from_numpy(s.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _check_shape(ctx, n, lanes, batch=1):
    shape = ctx.msm_last_shape()
    assert shape["path"] == "ordinary" and shape["prephase"] == 1 and shape["bucket_sets"] == 1 and shape["window_bits"] == 17, shape
    assert shape["batch"] == batch and shape["accumulate_variant"] == (2 if n <= 1 << 16 else 0), shape
    assert shape["reduce_lanes"] == lanes, shape


def run(ctx, style, vecs, n):
    """vecs: [(scalars, trapdoor value)]; a batch of them, the first one behind a commitment in flight, or the first one alone"""
    import plonkit_amd as pa
    if style == "batch3":
        dev = [_dev(s) for s, _ in vecs]
        got = list(ctx.msm_batch_dev(dev, n))
        _check_shape(ctx, n, 16, batch=3)
        for k, (_, want) in enumerate(vecs):
            assert np.array_equal(np.asarray(got[k]), want), (style, k)
    elif style == "inflight":
        other, want_other = expected("uniform", n, 5)
        d_other, d = _dev(other), _dev(vecs[0][0])
        ctx.msm_enqueue_dev(d_other, n)
        ctx.msm_enqueue_dev(d, n)
        got_other = pa.g1_sum_jacobian(ctx.msm_finish())
        got = pa.g1_sum_jacobian(ctx.msm_finish())
        _check_shape(ctx, n, 16)
        assert np.array_equal(np.asarray(got), vecs[0][1]), style
        assert np.array_equal(np.asarray(got_other), want_other), (style, "the commitment in flight before it")
    else:
        got = ctx.msm_dev(_dev(vecs[0][0]), n)
        _check_shape(ctx, n, 4)
        assert np.array_equal(np.asarray(got), vecs[0][1]), style


@pytest.mark.parametrize("n", [(1 << 15) + 1, (1 << 16) + 3])
@pytest.mark.parametrize("dist", DISTS)
def test_recoding_just_above_the_short_path(ctx, dist, n):
    run(ctx, "alone", [expected(dist, n, 1)], n)


@pytest.mark.parametrize("n", [(1 << 16) + 3, 1 << 17])
@pytest.mark.parametrize("style", ["batch3", "inflight", "alone"])
@pytest.mark.parametrize("dist", DISTS)
def test_reduction_by_16_lanes_and_by_quads(ctx, dist, style, n):
    # (a batch of three: the same distribution under three seeds — three equal vectors for the constant ones)
    run(ctx, style, [expected(dist, n, k + 1) for k in range(3)], n)


@pytest.mark.parametrize("n", [(1 << 16) + 3, 1 << 17])
def test_batch_of_three_different_vectors(ctx, n):
    """vector m of a batch has its own stretch of the canonical hand-over buffer and its own bucket set"""
    run(ctx, "batch3", [expected("one_hot", n, 2), expected("uniform", n, 1), expected("minus_one", n, 1)], n)
    run(ctx, "batch3", [expected("witness_like", n, 1), expected("ones", n, 1), expected("uniform", n, 3)], n)
