"""-m gpu: the inverse NTT over G1 (plonkit_amd/csrc/g1ntt.hip: dump-lagrange, every Lagrange-form key) on inputs that are NOT the consecutive
powers of a key, byte for byte against the CPU oracle (oracle.oracle_lib.g1_intt: serial radix-2 on Jacobian points, double-and-add) and, for the
sparse-spectrum family, against e_i Q computed without any transform.  The inputs and their reasoning are in tests/gen/g1_intt_check.py:

  * arbitrary points, every log_n from 0 to 12, then 14 and 16 — no stage at all, a lone scaling stage with jl = 0, sizes below one workgroup and
    below one normalisation group, both sides of the lane-layout switch at log_n 8 — with entries at infinity (first, last, an adjacent pair; a
    whole half);
  * the sparse-spectrum family, whose butterflies meet A == w B, A == -w B and points at infinity at every stage, on operands that come out of a
    scalar multiplication (ZZ, ZZZ far from 1), and whose outputs are at infinity singly, in runs and in whole normalisation groups;
  * the resident-key entry point on a stream that is not the context's, with a key of a general tau;
  * a small transform after a large one in the same scratch;
  * the two variants of the scalar multiplication that PLK_G1NTT_ISO selects (0: XYZZ table, 1: four effectively affine entries), each in a
    fresh process (the library reads the variable once).

tests/test_oracle_field.py validates the oracle's transform on the sparse family without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD
from tests.gen import g1_intt_check as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def _assert_same(got, want, what):
    i = gc.first_difference(got, want)
    assert i is None, "%s: first wrong index %d of %d\n  got  %s\n  want %s" % (what, i, got.shape[0], got[i].tolist(), want[i].tolist())


@pytest.mark.parametrize("kind", gc.ARBITRARY_KINDS)
@pytest.mark.parametrize("log_n", gc.ARBITRARY_LOG_N)
def test_arbitrary_points_match_the_oracle(ctx, log_n, kind):
    pts = gc.arbitrary_points(log_n, kind)
    inf = gc.infinity_indices(1 << log_n, kind)
    assert all(ol.g1_is_inf(pts[j]) for j in inf) and int(np.sum(~np.any(pts != 0, axis=1))) == len(inf)
    _assert_same(ctx.g1_intt(pts, log_n), ol.g1_intt(pts, log_n), "log_n %d, %s" % (log_n, kind))


@pytest.mark.parametrize("pattern", gc.SPARSE_PATTERNS)
@pytest.mark.parametrize("log_n", gc.SPARSE_LOG_N)
def test_sparse_spectrum_gives_the_chosen_scalars(ctx, log_n, pattern):
    pts, want, e = gc.sparse_case(log_n, pattern)
    assert [ol.g1_is_inf(p) for p in want] == [x == 0 for x in e]
    got = ctx.g1_intt(pts, log_n)
    _assert_same(got, want, "%s, log_n %d, against e_i Q" % (pattern, log_n))
    _assert_same(got, ol.g1_intt(pts, log_n), "%s, log_n %d, against the oracle's transform" % (pattern, log_n))


def test_resident_key_on_a_side_stream(ctx):
    """plk_g1_intt_srs_dev with the caller's stream: 2^13 points of a key generated on the GPU from a general tau (plk_srs_generate_fr, as
    test_srs_generation_with_a_general_tau does), against the oracle on the downloaded points"""
    import torch
    log_n = 13
    n = 1 << log_n
    tau = 0x1234567890abcdef1234567890abcdef1234567890abcdef % R_MOD
    ctx.srs_generate_fr(n, 0, ol.fr_mont(tau))
    pts = ctx.srs_download(0, n)
    for i in (0, 1, n - 1):
        assert np.array_equal(pts[i], ol.g1_mul(ol.g1_generator(), pow(tau, i, R_MOD))), i
    out = torch.zeros((n, 8), dtype=torch.int64, device="cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    assert side.cuda_stream != 0 and side.cuda_stream != torch.cuda.default_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.g1_intt_srs_dev(log_n, out.data_ptr(), stream=side)
    side.synchronize()
    _assert_same(out.cpu().numpy().view(np.uint64), ol.g1_intt(pts, log_n), "resident key, log_n %d" % log_n)


def test_a_small_transform_after_a_large_one_in_the_same_scratch():
    """2^10, 2^3, 2^10 on one context: the transform borrows the first commitment slot's scratch, which keeps the larger run's points"""
    import plonkit_amd as pa
    c = pa.Context(0)
    try:
        for log_n, pattern in ((10, "random_half_zero"), (3, "one_per_block_of_8"), (10, "alternating")):
            pts, want, _ = gc.sparse_case(log_n, pattern)
            _assert_same(c.g1_intt(pts, log_n), want, "%s, log_n %d" % (pattern, log_n))
    finally:
        c.close()


@pytest.mark.parametrize("iso", [0, 1])
def test_the_other_two_multiplication_variants(iso):
    """PLK_G1NTT_ISO=0 / 1 in a fresh process (tests/gen/g1_intt_check.py): the arbitrary-point cases up to 2^10 and the whole sparse family"""
    env = dict(os.environ, PLK_G1NTT_ISO=str(iso))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gen", "g1_intt_check.py"), "10"], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "PLK_G1NTT_ISO=%d: " % iso in r.stdout and "mismatches: 0" in r.stdout, r.stdout[-3000:]
