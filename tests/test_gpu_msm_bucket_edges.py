"""-m gpu: commitments whose buckets sit on the integer thresholds of the bucket schedule (plonkit_amd/csrc/msm_plan.h: slices of a bin,
entries per lane, the slot of a lane's run, the span of a bucket, owned tasks, folding a bin's tasks) and on the wave shortcuts of the
pre-phase and of the sort.  The cases and the (case, build) matrix are tests/gen/msm_bucket_cases.py; tests/test_msm_bucket_cases_host.py
has shown on the CPU that every case sits where its name says, so this file only runs them: every result bit-exact against the trapdoor
value, ONE host scalar multiplication of G (the key and the caller-supplied points are the tau = 42 powers).

Builds (gen.BUILDS; the smallest n that selects each), asserted through Context.msm_last_shape() and msm_last_no_inf() BEFORE the point is
looked at:
  owned       resident clean key, 2^15 + 1 terms: accumulate variant 2, fused recoding
  plain       resident clean key, 2^16 + 1 terms: the plain kernel without the infinity test
  plain_inf   the same on a key whose last point (beyond every commitment here) is at infinity: the plain kernel with the test
  bases13     msm_bases_dev at 4096 terms: c = 13, 64 bins, 20 bucket sets, the digit-array pre-phase, variant 2; cells in windows 0, 7, 19
  bases15     msm_bases_dev at 2^17 terms: c = 15, variant 0, infinity test on
Call styles: alone (a resident key reduces by quads; caller-supplied bases have 20 or 17 bucket sets and reduce with 32 lanes per task), a
batch of two (32 lanes per task), a batch of three with the case in the middle between two sparse uniform vectors (16 lanes per task, the
pair-product addition, the case's tasks behind a non-zero task_start, and three bins per lane in msm_scan_bins on a resident key).
One test function per (build, style) runs every case of the build; nothing is skipped."""
import numpy as np
import pytest

from oracle import oracle_lib as ol
from tests.gen import msm_bucket_cases as gen
from tests.test_msm_bases_plan_host import expected_shape

pytestmark = pytest.mark.gpu

KEY_N = 1 << 17
STYLES = {"alone": 1, "batch2": 2, "batch3_middle": 3}
LANES_RESIDENT = {1: 4, 2: 32, 3: 16}


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.uint64, order="C", copy=True).view(np.int64)).to("cuda:0")   # (a copy: the shared inputs are read-only)
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def world():
    """the key generated on the GPU once; three contexts: the clean key, the key with its last point at infinity, no key; and the same
    powers in device memory for the bases path"""
    import plonkit_amd as pa
    clean, inf, loose = pa.Context(0), pa.Context(0), pa.Context(0)
    try:
        clean.srs_generate(KEY_N, 0, 42)
        powers = clean.srs_download(0, KEY_N)
        late = powers.copy()
        late[KEY_N - 1] = 0
        inf.srs_upload(late)
        yield dict(owned=clean, plain=clean, plain_inf=inf, bases13=loose, bases15=loose, d_powers=_dev(powers))
    finally:
        for c in (clean, inf, loose):
            c.close()


def _montgomery(term_list, n):
    out = np.zeros((n, 4), dtype=np.uint64)
    by_value = {}
    for p, v in term_list:
        by_value.setdefault(v, []).append(p)
    for v, pos in by_value.items():
        out[np.array(pos, dtype=np.int64)] = ol.fr_mont(v)
    return out


_G = ol.g1_generator()
_INPUTS = {}


def _inputs(key, term_list, n):
    """(scalars in Montgomery form, expected point), computed once and left unchanged"""
    if key not in _INPUTS:
        s = _montgomery(term_list, n)
        s.setflags(write=False)
        _INPUTS[key] = (s, ol.g1_mul(_G, gen.expected_scalar(term_list, n)))
    return _INPUTS[key]


def _assert_build(ctx, build, n, batch, what):
    B = gen.BUILDS[build]
    shape = ctx.msm_last_shape()
    if B["bases"]:
        want = expected_shape(n, batch)
    else:
        want = dict(shape, path="ordinary", batch=batch, table_copies=15, window_bits=17, windows=15, bucket_sets=1, fine_bits=6, coarse_bins=1024,
                    prephase=1, reduce_lanes=LANES_RESIDENT[batch], pieces=1, piece_terms=n)
    want["accumulate_variant"] = B["variant"]
    assert (want["window_bits"], want["coarse_bins"], want["prephase"]) == (B["c"], B["nbins"], B["prephase"]), what
    assert shape == want, (what, {k: (shape[k], want[k]) for k in want if shape[k] != want[k]})
    assert ctx.msm_last_no_inf() is (build == "plain"), what


@pytest.mark.parametrize("style", list(STYLES))
@pytest.mark.parametrize("build", list(gen.BUILDS))
def test_bucket_edges(world, build, style):
    ctx, B, batch = world[build], gen.BUILDS[build], STYLES[style]
    ran = 0
    for case, k, b in gen.matrix():
        if b != build:
            continue
        n = case.n(build)
        s, want = _inputs((case.name, build), gen.terms(case, build, k), n)
        vecs, wants = [s], [want]
        if batch >= 2:                                               # the neighbours: sparse uniform vectors
            a, wa = _inputs(("neighbour", 1, n), gen.sparse_uniform(n, 1000 + n), n)
            vecs, wants = [s, a], [want, wa]
        if batch == 3:
            z, wz = _inputs(("neighbour", 2, n), gen.sparse_uniform(n, 2000 + n), n)
            vecs, wants = [a, s, z], [wa, want, wz]
        dev = [_dev(v) for v in vecs]
        if B["bases"]:
            got = ctx.msm_bases_dev(world["d_powers"], dev[0], n) if batch == 1 else ctx.msm_bases_batch_dev(world["d_powers"], dev, n)
        else:
            got = ctx.msm_dev(dev[0], n) if batch == 1 else ctx.msm_batch_dev(dev, n)
        _assert_build(ctx, build, n, batch, (case.name, build, style))
        got = np.asarray(got).reshape(batch, 8)
        for j in range(batch):
            assert np.array_equal(got[j], wants[j]), (case.name, build, style, "vector %d of %d" % (j, batch))
        ran += 1
    assert ran == sum(1 for _, _, b in gen.matrix() if b == build) and ran >= 26
