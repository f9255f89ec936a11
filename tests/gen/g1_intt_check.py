"""Inputs for the inverse NTT over G1 (plonkit_amd/csrc/g1ntt.hip) that are NOT the powers of a key, and a checker that runs them in a process
of its own.  tests/test_gpu_g1_intt.py and tests/test_oracle_field.py take the inputs from here; the same file run as a program,

    PLK_G1NTT_ISO=<0|1|2> python tests/gen/g1_intt_check.py [largest log_n of the arbitrary-point cases, default 10]

runs the arbitrary-point cases up to that size and the whole sparse-spectrum family through Context.g1_intt against the CPU oracle, stops at the
first mismatch with status 1 and prints `mismatches: 0` when there is none.  (The library reads PLK_G1NTT_ISO once per process: the two variants
of the scalar multiplication that are not the default can only be selected in a fresh process.)

Two families:

arbitrary points   random multiples of G, unrelated to each other, with some entries at infinity: `few` = the first, the last and an adjacent
                   pair; `half` = those and the whole upper half.

sparse spectrum    choose the OUTPUT scalars e_i first and feed in[j] = c_j Q with c_j = sum_i e_i omega^(i j) over Fr (the forward transform of
                   e, computed here with Python integers) for a fixed point Q = q G.  The inverse transform must return e_i Q, infinity where
                   e_i = 0 — known without any transform over the group.  Every partial result of the butterflies is then a multiple of Q by a
                   partial sum of a sparse spectrum: with one non-zero e_0 all inputs are EQUAL (every stage adds A to w B = A: the doubling
                   exit, and A - w B: the cancellation exit); with zeros in e, whole sub-transforms vanish (operands and results at infinity,
                   inside one normalisation group of 8 and across them).
"""
import concurrent.futures
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import numpy as np

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD

ARBITRARY_LOG_N = list(range(13)) + [14, 16]
ARBITRARY_KINDS = ("few", "half")
SPARSE_LOG_N = [1, 2, 3, 5, 6, 7, 8, 9, 11]
SPARSE_PATTERNS = ("all_zero", "first_only", "last_only", "middle_only", "all_equal", "alternating", "one_block_of_8", "one_per_block_of_8",
                   "random_half_zero")
Q_SCALAR = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100f00d % R_MOD     # Q = Q_SCALAR * G


def g_multiples(scalars):
    """uint64[len, 8]: k * G for every k, by the oracle's double-and-add; the calls are spread over threads (they release the interpreter lock)"""
    G = ol.g1_generator()
    out = np.zeros((len(scalars), 8), dtype=np.uint64)
    if not len(scalars):
        return out
    ol.g1_mul(G, 1)                                              # the library is loaded (and built) by one thread
    step = 64

    def chunk(lo):
        for i in range(lo, min(lo + step, len(scalars))):
            if scalars[i] % R_MOD:
                out[i] = ol.g1_mul(G, scalars[i] % R_MOD)
    with concurrent.futures.ThreadPoolExecutor(max_workers=ol.ncpu()) as ex:
        list(ex.map(chunk, range(0, len(scalars), step)))
    return out


def infinity_indices(n, kind):
    """entries of an arbitrary-point input that are set to infinity"""
    idx = set()
    if n >= 8:
        idx |= {0, n - 1, n // 3, n // 3 + 1}
    elif n >= 2:
        idx |= {0}
    if kind == "half":
        idx |= set(range(n // 2, n)) if n >= 2 else {0}
    return sorted(idx)


def arbitrary_points(log_n, kind, seed=0x6731):
    """uint64[n, 8]: independent random multiples of G, with the entries of infinity_indices at infinity"""
    n = 1 << log_n
    rng = random.Random(seed * 64 + log_n)
    inf = set(infinity_indices(n, kind))
    ks = [rng.randrange(1, R_MOD) for _ in range(n)]
    return g_multiples([0 if j in inf else k for j, k in enumerate(ks)])


def sparse_spectrum(log_n, pattern, seed=0x5a17):
    """the output scalars e (a list of n integers below r)"""
    n = 1 << log_n
    rng = random.Random(seed * 64 + log_n)
    v = [rng.randrange(1, R_MOD) for _ in range(n)]
    if pattern == "all_zero":
        keep = lambda i: False
    elif pattern == "first_only":
        keep = lambda i: i == 0
    elif pattern == "last_only":
        keep = lambda i: i == n - 1
    elif pattern == "middle_only":
        keep = lambda i: i == n // 2
    elif pattern == "all_equal":
        v = [v[0]] * n
        keep = lambda i: True
    elif pattern == "alternating":
        keep = lambda i: i % 2 == 1
    elif pattern == "one_block_of_8":                            # one normalisation group of g1ntt_to_affine holds points, the others infinity only
        block = (n // 8) // 2
        keep = lambda i: i // 8 == block
    elif pattern == "one_per_block_of_8":                        # every normalisation group: seven points at infinity and one that is not
        keep = lambda i: i % 8 == 5 % n
    elif pattern == "random_half_zero":
        zero = set(rng.sample(range(n), n // 2))
        keep = lambda i: i not in zero
    else:
        raise ValueError(pattern)
    return [v[i] if keep(i) else 0 for i in range(n)]


def forward_transform(e, log_n):
    """c_j = sum_i e_i omega^(i j) mod r, with Python integers: decimation in time, the recursion written out"""
    n = 1 << log_n
    assert len(e) == n
    if n == 1:
        return [e[0] % R_MOD]
    w = ol.omega(log_n)
    even, odd = forward_transform(e[0::2], log_n - 1), forward_transform(e[1::2], log_n - 1)
    out, t = [0] * n, 1
    for j in range(n // 2):
        x = t * odd[j] % R_MOD
        out[j], out[j + n // 2] = (even[j] + x) % R_MOD, (even[j] - x) % R_MOD
        t = t * w % R_MOD
    return out


def sparse_case(log_n, pattern):
    """-> (input points uint64[n, 8], expected output points uint64[n, 8], e)"""
    n = 1 << log_n
    e = sparse_spectrum(log_n, pattern)
    c = forward_transform(e, log_n)
    distinct = sorted(set(c) | set(e))
    at = dict((s, i) for i, s in enumerate(distinct))
    mult = g_multiples([s * Q_SCALAR % R_MOD for s in distinct])      # s * Q; the zero scalar: infinity
    pts, want = mult[[at[s] for s in c]], mult[[at[s] for s in e]]
    assert pts.shape == want.shape == (n, 8)
    return pts, want, e


def first_difference(got, want):
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    return None if bad.size == 0 else int(bad[0])


def main(argv):
    import plonkit_amd as pa
    top = int(argv[1]) if len(argv) > 1 else 10
    ctx = pa.Context(0)
    runs = 0

    def check(what, got, want):
        nonlocal runs
        runs += 1
        i = first_difference(got, want)
        if i is not None:
            print("MISMATCH %s: first wrong index %d of %d\n  got  %s\n  want %s" % (what, i, got.shape[0], got[i].tolist(), want[i].tolist()), flush=True)
            print("mismatches: 1")
            sys.exit(1)
    for log_n in [l for l in ARBITRARY_LOG_N if l <= top]:
        for kind in ARBITRARY_KINDS:
            pts = arbitrary_points(log_n, kind)
            check("arbitrary points, log_n %d, %s" % (log_n, kind), ctx.g1_intt(pts, log_n), ol.g1_intt(pts, log_n))
    for log_n in SPARSE_LOG_N:
        for pattern in SPARSE_PATTERNS:
            pts, want, _ = sparse_case(log_n, pattern)
            got = ctx.g1_intt(pts, log_n)
            check("sparse spectrum %s, log_n %d, against e_i Q" % (pattern, log_n), got, want)
            check("sparse spectrum %s, log_n %d, against the oracle's transform" % (pattern, log_n), got, ol.g1_intt(pts, log_n))
    ctx.close()
    print("PLK_G1NTT_ISO=%s: %d comparisons" % (os.environ.get("PLK_G1NTT_ISO", "(unset)"), runs))
    print("mismatches: 0")


if __name__ == "__main__":
    main(sys.argv)
