"""-m gpu: commitments against caller-supplied bases (plk_msm_g1_bases / _dev / _batch_dev) and the key check of points that are not
installed (plk_srs_check_points_dev): no resident key, no fixed-base table.

The expected sums come from a trapdoor, so no CPU MSM of the test's size is needed: P_j = 42^j G (plk_srs_generate + download on a second
context), the bases are a fixed pseudo-random permutation pi of the P_j with every 97th point negated, every 211th replaced by infinity
and a run of equal points (300 of them; a third of the vector below 900 terms), and the sum is (sum_i s_i eps_i 42^pi(i)) G by the
oracle's field arithmetic.  Up to 2^13 terms the oracle's own Pippenger is a second referee on bases with no structure (k_i G, k_i
random 64-bit).  Every case asserts Context.msm_last_shape() BEFORE it looks at the point (the shapes: tests/test_msm_bases_plan_host.py
expected_shape, written down by hand from DESIGN.md section 4.2c): sizes are the block edge of the front kernel (255 / 256 / 257), the
naive / pipeline switch (4095 / 4096), both ends of each window width (2^17 - 1 / 2^17, 2^19) and the owned / plain accumulate switch
(2^16 / 2^16 + 1).

srs_check_points_dev has plk_srs_check itself as its referee: the same points uploaded as the key of another context must give the same
(valid, bad_index) under the same seed.  The refused keys are built as in tests/test_gpu_key_check.py.

A call of more than 2^24 terms runs several passes, each with its own offset into the scalars and the bases: 2^24 + 4097 terms, built on the
device so that a pass which ignored either offset reads other points or other scalars; the checked call names a refused base as
offset + index, before and behind the seam, and the batch entry point refuses the length.

Checked bases "at 256 and 257 together": a vector of 257 terms has no index 257, so there the pair is 255 and 256 (it straddles the block
edge of the front kernel all the same); at 4096 terms it is 256 and 257."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol
from oracle.oracle_lib import Q_MOD, R_MOD
from tests.test_msm_bases_plan_host import FIELDS, expected_shape
from tests.test_gpu_key_check import _g2_encode, _twist_point_outside_the_subgroup

ERR_ARG, ERR_SIZE, ERR_SRS, ERR_FORMAT = 1, 2, 3, 6
NONE = 2**64 - 1
NMAX = 1 << 19
SIZES = [0, 1, 2, 255, 256, 257, 4095, 4096, (1 << 13) + 3, 1 << 16, (1 << 16) + 1, (1 << 17) - 1, 1 << 17, 1 << 19]
STYLES = ["uniform", "minus_one", "zeros_and_ones"]
SEEDS = [bytes([29 * k + 3]) * 32 for k in range(4)]             # four fixed seeds
NKEY = 1 << 12                                                   # size of the constructed keys
PATTERN = np.uint64(0x5a5a5a5a5a5a5a5a)


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.uint64, order="C", copy=True).view(np.int64)).to("cuda:0")   # (a copy: the shared cases are read-only)
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def ctx():
    """a context that never holds a key"""
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def powers():
    """P_j = 42^j G, j < 2^19, made on a context of their own"""
    import plonkit_amd as pa
    c = pa.Context(0)
    try:
        c.srs_generate(NMAX, 0, 42)
        return c.srs_download(0, NMAX)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ bases with known discrete logarithms
_CASES = {}


def trapdoor_bases(powers, n):
    """(bases [n, 8], exponent of each base, sign of each base: 1, -1 or 0 for infinity); computed once per size and left unchanged"""
    if n not in _CASES:
        rng = np.random.default_rng(97 * n + 1)
        e = rng.permutation(n)
        run, r0 = min(300, n // 3), n // 2
        if run >= 2:
            e[r0:r0 + run] = e[r0]                               # a run of equal points
        bases = np.ascontiguousarray(powers[e])
        eps = np.ones(n, dtype=np.int64)
        for i in range(96, n, 97):                               # every 97th negated
            bases[i] = ol.g1_neg(bases[i])
            eps[i] = -1
        bases[210::211] = 0                                      # every 211th at infinity
        eps[210::211] = 0
        bases.setflags(write=False)
        _CASES[n] = (bases, e, eps)
    return _CASES[n]


def trapdoor_sum(s, e, eps):
    """(sum_i s_i eps_i 42^e_i) G"""
    n = len(e)
    if n == 0:
        return np.zeros(8, dtype=np.uint64)
    t = np.array(s, dtype=np.uint64, copy=True)
    neg = eps == -1
    if neg.any():
        t[neg] = ol.vsub(np.zeros((int(neg.sum()), 4), dtype=np.uint64), np.ascontiguousarray(t[neg]))
    t[eps == 0] = 0
    _, first = np.unique(e, return_index=True)                   # every exponent once: a polynomial in 42 ...
    c = np.zeros((n, 4), dtype=np.uint64)
    c[e[first]] = t[first]
    total = ol.poly_eval(c, 42)
    rest = np.setdiff1d(np.arange(n), first)                     # ... and the rest of the run, which shares one exponent
    if rest.size:
        assert len(set(e[rest].tolist())) == 1
        total += sum(ol.fr_ints(np.ascontiguousarray(t[rest]))) * pow(42, int(e[rest[0]]), R_MOD)
    return ol.g1_mul(ol.g1_generator(), total % R_MOD)


def scalars(style, n, seed):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    u[:, 3] &= np.uint64((1 << 60) - 1)                          # < 2^252 < r: valid Montgomery residues
    if style == "uniform":
        return u
    if style == "minus_one":
        return np.tile(ol.fr_mont(R_MOD - 1), (n, 1))
    assert style == "zeros_and_ones"                             # 45 % zero, 45 % one, 10 % uniform: hot buckets
    sel = rng.integers(0, 20, size=n)
    u[sel < 9] = 0
    u[(sel >= 9) & (sel < 18)] = ol.fr_mont(1)
    return u


def _assert_shape(ctx, n, batch, what):
    shape, want = ctx.msm_last_shape(), expected_shape(n, batch)
    assert shape == want, (what, {k: (shape[k], want[k]) for k in FIELDS if shape[k] != want[k]})


@pytest.mark.parametrize("n", SIZES, ids=lambda n: "n%d" % n)
def test_shape_then_trapdoor_sum(ctx, powers, n):
    bases, e, eps = trapdoor_bases(powers, n)
    d_bases = _dev(bases) if n else 0
    for k, style in enumerate(STYLES):
        s = scalars(style, n, 1000 * k + n)
        d_s = _dev(s) if n else 0
        got = ctx.msm_bases_dev(d_bases, d_s, n, check=(k == 1))             # (the bases are sound: checking changes nothing)
        _assert_shape(ctx, n, 1, (n, style))
        assert np.array_equal(got, trapdoor_sum(s, e, eps)), (n, style)
    if n == 0:
        assert ol.g1_is_inf(got)


# ------------------------------------------------------------------------------------------------ the oracle's own MSM, both entry points
@pytest.fixture(scope="module")
def loose_bases():
    """k_i G with random 64-bit k_i; one point at infinity"""
    rng = np.random.default_rng(5)
    g = ol.g1_generator()
    pts = np.stack([ol.g1_mul(g, int(k)) for k in rng.integers(1, 1 << 63, size=1 << 13, dtype=np.uint64)])
    pts[77] = 0
    return pts


@pytest.mark.parametrize("n", [1, 257, 4095, 4096, 1 << 13], ids=lambda n: "n%d" % n)
def test_against_the_oracle_msm_host_and_device_pointers(ctx, loose_bases, n):
    b = np.ascontiguousarray(loose_bases[:n])
    s = scalars("uniform", n, 31 + n)
    s[n // 2] = 0
    want = ol.msm(b, s)
    got_dev = ctx.msm_bases_dev(_dev(b), _dev(s), n)
    _assert_shape(ctx, n, 1, n)
    assert np.array_equal(got_dev, want)
    got_host = ctx.msm_bases(b, s, check=True)
    _assert_shape(ctx, n, 1, n)
    assert np.array_equal(got_host, want)


# ------------------------------------------------------------------------------------------------ batch
@pytest.mark.parametrize("n", [4096, (1 << 16) + 1], ids=lambda n: "n%d" % n)
def test_batch_equals_single_calls(ctx, powers, n):
    import plonkit_amd as pa
    bases, e, eps = trapdoor_bases(powers, n)
    d_bases = _dev(bases)
    vecs = [scalars(STYLES[k % 3], n, 7000 + 13 * k + n) for k in range(8)]
    dev = [_dev(v) for v in vecs]
    single = []
    for k in range(8):
        single.append(ctx.msm_bases_dev(d_bases, dev[k], n))
        assert np.array_equal(single[k], trapdoor_sum(vecs[k], e, eps)), k
    for count in (2, 3, 8):
        got = ctx.msm_bases_batch_dev(d_bases, dev[:count], n)
        _assert_shape(ctx, n, count, (n, count))
        assert got.shape == (count, 8)
        for k in range(count):
            assert np.array_equal(got[k], single[k]), (count, k)
    for count in (0, 9):
        with pytest.raises(pa.PlkError) as err:
            ctx.msm_bases_batch_dev(d_bases, (dev + dev)[:count], n)
        assert err.value.code == ERR_ARG


# ------------------------------------------------------------------------------------------------ no key, arguments
def test_no_key_resident_and_argument_errors(powers):
    import plonkit_amd as pa
    L = pa.lib()
    c = pa.Context(0)
    try:
        n = 5000
        bases, e, eps = trapdoor_bases(powers, n)
        s = scalars("uniform", n, 3)
        d_b, d_s = _dev(bases), _dev(s)
        assert np.array_equal(c.msm_bases_dev(d_b, d_s, n), trapdoor_sum(s, e, eps))
        assert c.srs_size() == 0
        with pytest.raises(pa.PlkError) as err:
            c.msm_dev(d_s, n)
        assert err.value.code == ERR_SRS
        assert np.array_equal(c.msm_bases(bases, s), trapdoor_sum(s, e, eps))   # and again after the refusal
        out, bad = np.full(8, PATTERN, dtype=np.uint64), ctypes.c_uint64(5)
        o = out.ctypes.data_as(ctypes.c_void_p)
        bp, sp = ctypes.c_void_p(d_b.data_ptr()), ctypes.c_void_p(d_s.data_ptr())
        N = ctypes.c_uint64(n)
        for flags in (2, 4, 0x80000001):                                         # unknown flag bits
            assert L.plk_msm_g1_bases_dev(c._h, bp, sp, N, ctypes.c_uint32(flags), o, ctypes.byref(bad), None) == ERR_ARG
        assert L.plk_msm_g1_bases_dev(c._h, ctypes.c_void_p(d_b.data_ptr() + 8), sp, N, ctypes.c_uint32(0), o, ctypes.byref(bad), None) == ERR_ARG   # alignment
        assert L.plk_msm_g1_bases_dev(c._h, bp, ctypes.c_void_p(d_s.data_ptr() + 8), N, ctypes.c_uint32(0), o, ctypes.byref(bad), None) == ERR_ARG
        assert L.plk_msm_g1_bases_dev(c._h, None, sp, N, ctypes.c_uint32(0), o, ctypes.byref(bad), None) == ERR_ARG
        assert L.plk_msm_g1_bases_dev(c._h, bp, None, N, ctypes.c_uint32(0), o, ctypes.byref(bad), None) == ERR_ARG
        assert L.plk_msm_g1_bases_dev(c._h, bp, sp, N, ctypes.c_uint32(0), None, ctypes.byref(bad), None) == ERR_ARG
        ptrs = (ctypes.c_void_p * 2)(sp, sp)
        assert L.plk_msm_g1_bases_batch_dev(c._h, bp, ptrs, ctypes.c_uint32(2), ctypes.c_uint64((1 << 24) + 1), ctypes.c_uint32(0), o, None, None) == ERR_SIZE
        assert np.all(out == PATTERN)
        assert L.plk_msm_g1_bases_dev(c._h, bp, sp, N, ctypes.c_uint32(0), o, None, None) == 0               # bad_out may be NULL
        assert np.array_equal(out, trapdoor_sum(s, e, eps))
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ resident state
def test_resident_key_and_table_are_untouched(powers):
    import plonkit_amd as pa
    c = pa.Context(0)
    try:
        c.srs_generate(1 << 16, 0, 42)
        v12, v16 = scalars("uniform", 1 << 12, 41), scalars("uniform", 1 << 16, 43)
        d12, d16 = _dev(v12), _dev(v16)

        def resident():
            p12 = c.msm_dev(d12, 1 << 12)
            s12 = c.msm_last_shape()
            p16 = c.msm_dev(d16, 1 << 16)
            return p12, s12, p16, c.msm_last_shape()

        before = resident()
        assert before[1]["path"] == "short" and before[1]["table_copies"] == 15 and before[3]["path"] == "ordinary" and before[3]["table_copies"] == 15
        for n in (100, 4095, 4096, (1 << 16) + 1):
            bases, e, eps = trapdoor_bases(powers, n)
            s = scalars("uniform", n, 47 + n)
            assert np.array_equal(c.msm_bases_dev(_dev(bases), _dev(s), n, check=(n == 4096)), trapdoor_sum(s, e, eps)), n
            _assert_shape(c, n, 1, n)
        after = resident()
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
        assert after[1] == before[1] and after[3] == before[3]
        assert np.array_equal(c.srs_download(0, 16), powers[:16]) and c.srs_size() == 1 << 16
        # a borrower may commit to its own points; the loan stands
        other = pa.Context(0)
        try:
            other.share_srs_from(c)
            bases, e, eps = trapdoor_bases(powers, 4096)
            s = scalars("uniform", 4096, 53)
            assert np.array_equal(other.msm_bases(bases, s), trapdoor_sum(s, e, eps))
            assert np.array_equal(c.msm_bases(bases, s), trapdoor_sum(s, e, eps))          # and so may the lender
            assert np.array_equal(other.msm_dev(d12, 1 << 12), before[0]) and other.msm_last_shape() == before[1]
            with pytest.raises(pa.PlkError) as err:
                c.srs_generate(1024, 0, 42)                                               # the lender still refuses to replace its key
            assert err.value.code == ERR_ARG
        finally:
            other.close()
    finally:
        c.close()


def test_refused_while_a_commitment_is_in_flight(powers):
    import plonkit_amd as pa
    c = pa.Context(0)
    try:
        n = 4096
        c.srs_generate(n, 0, 42)
        bases, e, eps = trapdoor_bases(powers, n)
        s = scalars("uniform", n, 59)
        d_b, d_s = _dev(bases), _dev(s)
        g2 = pa.crs42_g2_bytes()
        d_key = _dev(powers[:n])
        c.msm_enqueue_dev(d_s, n)
        calls = [lambda: c.msm_bases(bases, s), lambda: c.msm_bases_dev(d_b, d_s, n), lambda: c.msm_bases_batch_dev(d_b, [d_s, d_s], n),
                 lambda: c.srs_check_points_dev(d_key, n, g2, seed=SEEDS[0])]
        for call in calls:
            with pytest.raises(pa.PlkError) as err:
                call()
            assert err.value.code == ERR_ARG and "in flight" in str(err.value)
        first = pa.g1_sum_jacobian(c.msm_finish())
        assert np.array_equal(first, ol.g1_mul(ol.g1_generator(), ol.poly_eval(s, 42)))
        want = trapdoor_sum(s, e, eps)
        assert np.array_equal(calls[0](), want) and np.array_equal(calls[1](), want)
        assert np.array_equal(calls[2](), np.stack([want, want]))
        assert calls[3]() == (True, None)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ checked bases
def _raw_add(limbs, k):
    """the four limbs as an integer + k, not reduced"""
    return ol.int_to_limbs(ol.limbs_to_int(limbs) + k)


def _spoil(bases, kind, n):
    """(spoiled copy, refused indexes)"""
    b = np.array(bases, copy=True)
    if kind == "first":
        where = [0]
    elif kind == "last":
        where = [n - 1]
    elif kind == "pair":
        where = [256, 257] if n > 257 else [255, 256]
    else:
        where = [n // 2]
    for i in where:
        if kind == "x_is_q":                                     # out of range: x = q as raw limbs
            b[i, :4] = ol.int_to_limbs(Q_MOD)
        elif kind == "zero_one":                                 # (0, 1): neither infinity nor on the curve
            b[i] = 0
            b[i, 4] = 1
        else:                                                    # y + 1: off the curve
            assert b[i].any()
            b[i, 4:] = _raw_add(b[i, 4:], 1)
    return b, where


@pytest.mark.parametrize("n", [257, 4096], ids=lambda n: "n%d" % n)
@pytest.mark.parametrize("kind", ["first", "last", "pair", "x_is_q", "zero_one"])
def test_checked_bases(ctx, powers, n, kind):
    import plonkit_amd as pa
    L = pa.lib()
    bases, e, eps = trapdoor_bases(powers, n)
    for i in (0, n - 1, 255, 256, 257, n // 2):
        assert i >= n or eps[i] != 0, "the spoiled indexes must hold points"
    spoiled, where = _spoil(bases, kind, n)
    s = scalars("uniform", n, 61 + n)
    d_bad, d_s = _dev(spoiled), _dev(s)
    # a kernel has run before (the shape of the last commitment must not change by a refused call)
    mended = np.array(spoiled, copy=True)
    mended[where] = 0
    eps_mended = eps.copy()
    eps_mended[where] = 0
    want = trapdoor_sum(s, e, eps_mended)
    assert np.array_equal(ctx.msm_bases_dev(_dev(mended), d_s, n, check=True), want)
    _assert_shape(ctx, n, 1, (n, kind, "mended"))
    out, bad = np.full(8, PATTERN, dtype=np.uint64), ctypes.c_uint64(5)
    rc = L.plk_msm_g1_bases_dev(ctx._h, ctypes.c_void_p(d_bad.data_ptr()), ctypes.c_void_p(d_s.data_ptr()), ctypes.c_uint64(n), ctypes.c_uint32(1),
                                out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(bad), None)
    assert rc == ERR_FORMAT and bad.value == where[0] and np.all(out == PATTERN)
    assert "point not on curve" in pa.last_error()
    with pytest.raises(pa.PlkError) as err:                      # the host-pointer entry point and the Python layer
        ctx.msm_bases(spoiled, s, check=True)
    assert err.value.code == ERR_FORMAT and err.value.bad_index == where[0]
    with pytest.raises(pa.PlkError) as err:
        ctx.msm_bases_batch_dev(d_bad, [d_s, d_s], n, check=True)
    assert err.value.code == ERR_FORMAT and err.value.bad_index == where[0]
    # unchecked: taken on trust — some point, no index
    bad = ctypes.c_uint64(5)
    rc = L.plk_msm_g1_bases_dev(ctx._h, ctypes.c_void_p(d_bad.data_ptr()), ctypes.c_void_p(d_s.data_ptr()), ctypes.c_uint64(n), ctypes.c_uint32(0),
                                out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(bad), None)
    assert rc == 0 and bad.value == NONE and not np.all(out == PATTERN)
    _assert_shape(ctx, n, 1, (n, kind, "unchecked"))


# ------------------------------------------------------------------------------------------------ two passes
def test_two_passes_with_their_own_offsets(powers):
    """2^24 + 4097 terms: a pass of 2^24 and one of 4097 (the pipeline, not the naive kernel), each with its own offset into the scalars and
    the bases.  Everything is built on the device: the first pass's bases are P_0 .. P_65535 tiled 256 times under u in the even and w in
    the odd blocks, the tail is P_1000 .. P_5096 under v — a pass that ignored its base offset would read P_0 .. instead of P_1000 .., one
    that ignored its scalar offset u instead of v.  Expected: (128 (u(42) + w(42)) + 42^1000 v(42)) G.  About 2.6 GiB of device memory."""
    import torch
    import plonkit_amd as pa
    L = pa.lib()
    BLOCK, TILES, FIRST, TAIL, SHIFT = 1 << 16, 256, 1 << 24, 4097, 1000
    n = FIRST + TAIL
    u, w, v = scalars("uniform", BLOCK, 71), scalars("uniform", BLOCK, 73), scalars("uniform", TAIL, 79)
    total = (128 * (ol.poly_eval(u, 42) + ol.poly_eval(w, 42)) + pow(42, SHIFT, R_MOD) * ol.poly_eval(v, 42)) % R_MOD
    want = ol.g1_mul(ol.g1_generator(), total)
    d_bases = torch.empty((n, 8), dtype=torch.int64, device="cuda:0")
    d_bases[:FIRST].view(TILES, BLOCK, 8).copy_(_dev(powers[:BLOCK]))
    d_bases[FIRST:].copy_(_dev(powers[SHIFT:SHIFT + TAIL]))
    d_s = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    pairs = d_s[:FIRST].view(TILES // 2, 2, BLOCK, 4)
    pairs[:, 0].copy_(_dev(u))
    pairs[:, 1].copy_(_dev(w))
    d_s[FIRST:].copy_(_dev(v))
    torch.cuda.synchronize()
    c = pa.Context(0)
    try:
        def good(check):
            got = c.msm_bases_dev(d_bases, d_s, n, check=check)
            shape, last = c.msm_last_shape(), expected_shape(TAIL, 1)               # the record of the last pass, and of the call
            last.update(pieces=2, piece_terms=FIRST)
            assert shape == last, {k: (shape[k], last[k]) for k in FIELDS if shape[k] != last[k]}
            assert np.array_equal(got, want), "check=%s" % check

        def spoil(index, source):
            row = np.array(powers[source], copy=True)
            assert row.any()
            row[4:] = _raw_add(row[4:], 1)                                          # y + 1: off the curve
            d_bases[index].copy_(_dev(row))

        def mend(index, source):
            d_bases[index].copy_(_dev(powers[source]))

        good(False)
        good(True)
        before, after = FIRST - 1, FIRST + 5                                        # the last base of the first pass, the sixth of the second
        src = {before: BLOCK - 1, after: SHIFT + 5}
        for k, (bad, named) in enumerate((((after,), after), ((before,), before), ((before, after), before))):
            for i in bad:
                spoil(i, src[i])
            with pytest.raises(pa.PlkError) as err:
                c.msm_bases_dev(d_bases, d_s, n, check=True)
            assert err.value.code == ERR_FORMAT and err.value.bad_index == named, (bad, err.value.bad_index)
            for i in bad:
                mend(i, src[i])
            good(k != 1)
        # the batch entry point does not split: refused before anything is launched
        shape = c.msm_last_shape()
        out, bad = np.full((2, 8), PATTERN, dtype=np.uint64), ctypes.c_uint64(5)
        ptrs = (ctypes.c_void_p * 2)(d_s.data_ptr(), d_s.data_ptr())
        rc = L.plk_msm_g1_bases_batch_dev(c._h, ctypes.c_void_p(d_bases.data_ptr()), ptrs, ctypes.c_uint32(2), ctypes.c_uint64(n), ctypes.c_uint32(0),
                                          out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(bad), None)
        assert rc == ERR_SIZE and np.all(out == PATTERN) and bad.value == NONE and c.msm_last_shape() == shape
        with pytest.raises(pa.PlkError) as err:
            c.msm_bases_batch_dev(d_bases, [d_s, d_s], n, check=True)
        assert err.value.code == ERR_SIZE and c.msm_last_shape() == shape
    finally:
        c.close()
        del d_bases, d_s, pairs
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the key check of points that are no key
@pytest.fixture(scope="module")
def referee():
    """plk_srs_check on the same points made resident: another context"""
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g2_42():
    import plonkit_amd as pa
    return pa.crs42_g2_bytes()


def _same_verdicts(ctx, referee, pts, g2, expect_valid, expect_link=None):
    n = pts.shape[0]
    d = _dev(pts)
    referee.srs_upload(pts)
    for seed in SEEDS:
        for locate in (False, True):
            got = ctx.srs_check_points_dev(d, n, g2, seed=seed, locate=locate)
            assert got == referee.srs_check(g2, seed=seed, locate=locate), (seed[:1].hex(), locate)
            assert got[0] is expect_valid
            if locate and not expect_valid:
                assert got[1] == expect_link
    assert ctx.srs_check_points_dev(d, n, g2, locate=True) == ((True, None) if expect_valid else (False, expect_link))   # OS randomness
    assert ctx.srs_size() == 0                                   # nothing was installed


def test_check_points_golden_key(ctx, referee, golden_dir):
    import torch
    raw = open(os.path.join(golden_dir, "setup_2pow10.key"), "rb").read()
    file_bytes = torch.from_numpy(np.frombuffer(raw[8:8 + 64 * 1024], dtype=np.uint8).copy()).to("cuda:0")
    pts = torch.zeros((1024, 8), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.g1_decode_dev(file_bytes, 1024, pts)
    g2 = raw[-256:]
    n, g2_ref = referee.srs_load_key(raw)
    assert n == 1024 and g2_ref == g2
    for seed in SEEDS:
        for locate in (False, True):
            assert ctx.srs_check_points_dev(pts, 1024, g2, seed=seed, locate=locate) == referee.srs_check(g2, seed=seed, locate=locate) == (True, None)
    assert ctx.msm_last_shape() == expected_shape(1024, 1)       # the commitment went through the bases path: naive, no table
    assert np.array_equal(pts.cpu().numpy().view(np.uint64), referee.srs_download(0, 1024))


def _tampered(kind, k, pts42, pts43):
    """(points, lowest broken link): the constructions of tests/test_gpu_key_check.py"""
    pts = pts42.copy()
    if kind == "repeat":                                         # P_k := P_{k-1}
        pts[k] = pts42[k - 1]
    elif kind == "negate":                                       # P_k := -P_k
        pts[k] = ol.g1_neg(pts42[k])
    elif kind == "swap":                                         # P_k <-> P_{k+1}
        pts[k], pts[k + 1] = pts42[k + 1], pts42[k]
    elif kind == "splice":                                       # first k points of tau = 42, the rest 43^i G: every later link is broken too
        pts[k:] = pts43[k:]
    return pts, k - 1


@pytest.fixture(scope="module")
def pts43(referee):
    referee.srs_generate(NKEY, 0, 43)
    return referee.srs_download(0, NKEY)


def test_check_points_valid_key(ctx, referee, powers, g2_42):
    _same_verdicts(ctx, referee, np.ascontiguousarray(powers[:NKEY]), g2_42, True)
    assert ctx.msm_last_shape() == expected_shape(NKEY, 1)       # one copy: no table was built for it


@pytest.mark.parametrize("kind,k", [("repeat", NKEY // 2), ("negate", 1), ("swap", NKEY - 2), ("splice", 1357)])
def test_check_points_tampered_keys(ctx, referee, powers, pts43, g2_42, kind, k):
    pts, link = _tampered(kind, k, np.ascontiguousarray(powers[:NKEY]), pts43)
    _same_verdicts(ctx, referee, pts, g2_42, False, link)


def test_check_points_first_point_at_infinity_and_one_point(ctx, referee, powers, g2_42):
    pts = np.ascontiguousarray(powers[:NKEY]).copy()
    pts[0] = 0
    d = _dev(pts)
    referee.srs_upload(pts)
    for locate in (False, True):
        assert ctx.srs_check_points_dev(d, NKEY, g2_42, seed=SEEDS[0], locate=locate) == referee.srs_check(g2_42, seed=SEEDS[0], locate=locate) == (False, 0)
    one = _dev(powers[:1])                                       # n = 1: only the conditions on P_0 and g2
    referee.srs_upload(powers[:1])
    assert ctx.srs_check_points_dev(one, 1, g2_42, seed=SEEDS[1]) == referee.srs_check(g2_42, seed=SEEDS[1]) == (True, None)
    assert ctx.srs_check_points_dev(_dev(pts[:1]), 1, g2_42, seed=SEEDS[1]) == (False, 0)


def test_check_points_wrong_g2_and_arguments(ctx, referee, powers, g2_42):
    import plonkit_amd as pa
    L = pa.lib()
    pts = np.ascontiguousarray(powers[:NKEY])
    d = _dev(pts)
    referee.srs_upload(pts)
    q0, q1 = g2_42[:128], g2_42[128:]
    sb = _g2_encode(_twist_point_outside_the_subgroup())         # on the twist, outside the order-r subgroup: a verdict
    for pair in (sb + q1, q0 + sb, q1 + q0):
        for locate in (False, True):
            got = ctx.srs_check_points_dev(d, NKEY, pair, seed=SEEDS[0], locate=locate)
            assert got == referee.srs_check(pair, seed=SEEDS[0], locate=locate) and got[0] is False
    assert ctx.srs_check_points_dev(d, NKEY, sb + q1, seed=SEEDS[0], locate=True) == (False, None)
    off = bytearray(g2_42)                                       # one byte flipped: off the twist, an argument error
    off[127] ^= 1
    with pytest.raises(pa.PlkError) as err:
        ctx.srs_check_points_dev(d, NKEY, bytes(off), seed=SEEDS[0])
    assert err.value.code == ERR_ARG and "G2 point not on the twist" in str(err.value)
    with pytest.raises(pa.PlkError) as ref_err:
        referee.srs_check(bytes(off), seed=SEEDS[0])
    assert ref_err.value.code == ERR_ARG
    valid, bad = ctypes.c_int32(7), ctypes.c_uint64(7)
    p, N = ctypes.c_void_p(d.data_ptr()), ctypes.c_uint64(NKEY)
    for flags in (1, 4, 3, 0x80000000):
        assert L.plk_srs_check_points_dev(ctx._h, p, N, g2_42, SEEDS[0], ctypes.c_uint32(flags), ctypes.byref(valid), ctypes.byref(bad), None) == ERR_ARG
    assert L.plk_srs_check_points_dev(ctx._h, None, N, g2_42, SEEDS[0], ctypes.c_uint32(0), ctypes.byref(valid), ctypes.byref(bad), None) == ERR_ARG
    assert L.plk_srs_check_points_dev(ctx._h, ctypes.c_void_p(d.data_ptr() + 8), N, g2_42, SEEDS[0], ctypes.c_uint32(0), ctypes.byref(valid), ctypes.byref(bad), None) == ERR_ARG
    assert L.plk_srs_check_points_dev(ctx._h, p, N, None, SEEDS[0], ctypes.c_uint32(0), ctypes.byref(valid), ctypes.byref(bad), None) == ERR_ARG
    assert L.plk_srs_check_points_dev(ctx._h, p, N, g2_42, SEEDS[0], ctypes.c_uint32(0), None, ctypes.byref(bad), None) == ERR_ARG
    assert L.plk_srs_check_points_dev(ctx._h, p, ctypes.c_uint64(0), g2_42, SEEDS[0], ctypes.c_uint32(0), ctypes.byref(valid), ctypes.byref(bad), None) == ERR_SRS
    assert L.plk_srs_check_points_dev(ctx._h, p, N, g2_42, SEEDS[0], ctypes.c_uint32(2), ctypes.byref(valid), None, None) == 0 and valid.value == 1   # bad_out may be NULL


def test_check_points_beside_a_resident_key(powers, pts43, g2_42):
    """a candidate key is judged on the context that holds the key in use: that key still passes plk_srs_check afterwards and its next
    commitment has the shape it had before"""
    import plonkit_amd as pa
    c = pa.Context(0)
    try:
        c.srs_generate(NKEY, 0, 42)
        s = scalars("uniform", NKEY, 67)
        d_s = _dev(s)
        point, shape = c.msm_dev(d_s, NKEY), c.msm_last_shape()
        assert shape["table_copies"] == 15
        assert c.srs_check_points_dev(_dev(pts43), NKEY, g2_42, seed=SEEDS[2], locate=True) == (False, 0)      # tau = 43 against 42's G2 section
        assert c.msm_last_shape()["table_copies"] == 1
        assert c.srs_check_points_dev(_dev(powers[:NKEY]), NKEY, g2_42, seed=SEEDS[2]) == (True, None)
        assert c.srs_check(g2_42, seed=SEEDS[3], locate=True) == (True, None)
        assert np.array_equal(c.srs_download(0, NKEY), powers[:NKEY])
        assert np.array_equal(c.msm_dev(d_s, NKEY), point) and c.msm_last_shape() == shape
    finally:
        c.close()
