"""-m gpu: every dispatch shape of the MSM, asserted before the answer is looked at.

msm_plan_pass / msm_plan_fallback / msm_plan_call (plonkit_amd/csrc/msm_plan.h; msm.hip launches what they plan) choose a commitment's kernels
from its length, its batch size, the key's size, what is resident and what is in flight.  ROWS below is one table of
(key, terms, base_offset, batch, call style, scalars, expected shape): per row the test first asserts that
Context.msm_last_shape() (plk_msm_last_shape, a diagnostic) reports the expected shape and then that the result is the
tau = 42 trapdoor answer (sum_i s_i 42^(off + i)) * G (Horner in the oracle's C arithmetic, ol.msm as well up to 5000 terms).

The expected shapes are written by hand from the rules in msm_plan.h's comments and DESIGN.md section 4.2, never read from the library
(tests/test_msm_plan_host.py checks the same table against the plan alone, without a GPU):
  * table copies of a key: 15 while 15 x 64 B x points <= 32 GiB (up to 35 791 394 points), else 1;
  * short path (msm_small.hip): 1 .. 2^15 terms on a 15-copy key, if the commitment has >= 4096 terms, or the key has <= 2^21
    points, or the 15 copies are resident already; otherwise fewer than 4096 terms take one double-and-add per term (naive);
  * window bits: 17 with the table; without it 13 below 2^17 terms, 15 below 2^19, 17 from there; windows = 254 // c + 1
    (20 / 17 / 15); buckets per task 2^6, so coarse bins = 2^(c - 7) (64 / 256 / 1024);
  * copies a commitment addresses: the largest divisor of 15 with copies * 2^ceil(log2 terms) <= 2^24: 15 up to 2^20 terms, 5 up to
    2^21, 3 up to 2^22, 1 above; bucket sets = windows / copies;
  * pre-phase: fused recoding for one bucket set of 17-bit windows, the digit array otherwise;
  * accumulate variant 2 (lanes own buckets) up to 2^16 terms, 0 above;
  * bucket reduction: quads for ONE bucket set (batch x sets == 1) with nothing else in flight, else 16 lanes per task for a
    batch >= 3 or with another commitment in flight, else 32;
  * plk_msm_g1_dev / _partial_dev: from 2^23 terms on a 15-copy key 2^20-term pieces, three in flight; otherwise passes of 2^24.
A threshold that moves fails the shape assertion of the rows next to it.  (Reading the rules this way, a 5000-term tail of a long
commitment takes the SHORT path — 4096 .. 2^15 terms on a 15-copy key; the tail for the 2^20-shaped kernels is the 40000-term row.)

Keys: K16 2^16 points; K22 2^22 (its rows are ONE sequence on a fresh context: 100 terms are naive before and short after the
first long commitment); K24 2^24 (the size of tests/test_gpu_large.py); K1COPY 2^25 + 2^22 points, 2.25 GiB + the same in the
accumulation's domain, no shifted copies.  Scalars: uniform with a third zeroed, except the distribution cells on K1COPY at 5000,
2^16, 2^18 + 7 and 2^19 terms (ones, r - 1, witness-like, below 4, top bits set, all zero, one-hot), which are complete: no cell
was thinned.  test_cover_of_the_matrix (no GPU) fails if a shape class loses its last row; test_design_md_table (no GPU) keeps
DESIGN.md's table of covered shapes equal to this one (python tests/test_gpu_msm_shapes.py prints it)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD

KEYS = {"K16": 1 << 16, "K22": 1 << 22, "K24": 1 << 24, "K1COPY": (1 << 25) + (1 << 22)}
FIELDS = ("path", "batch", "table_copies", "window_bits", "windows", "bucket_sets", "fine_bits", "coarse_bins", "accumulate_variant", "prephase",
          "reduce_lanes", "pieces", "piece_terms")
FUSED, DIGITS = 1, 2
WINDOWS_AND_BINS = {13: (20, 64), 15: (17, 256), 17: (15, 1024)}      # 254 // c + 1 windows, 2^(c - 7) coarse bins


def _shape(path, n, batch=1, copies=0, pieces=1, piece_terms=None, **kw):
    d = dict.fromkeys(FIELDS, 0)
    d.update(path=path, batch=batch, table_copies=copies, pieces=pieces, piece_terms=n if piece_terms is None else piece_terms)
    d.update(kw)
    return d


def naive(n, batch=1, **kw):
    return _shape("naive", n, batch, 1, **kw)


def short(n, batch=1, **kw):
    return _shape("short", n, batch, 15, **kw)


def ordinary(n, c, sets, copies, variant, prephase, lanes, batch=1, path="ordinary", **kw):
    windows, bins = WINDOWS_AND_BINS[c]
    return _shape(path, n, batch, copies, window_bits=c, windows=windows, bucket_sets=sets, fine_bits=6, coarse_bins=bins,
                  accumulate_variant=variant, prephase=prephase, reduce_lanes=lanes, **kw)


P15, P16, P17, P18, P19, P20, P21, P22, P23, P24 = (1 << k for k in range(15, 25))
ROWS = []


def row(key, n, expect, off=0, batch=1, style="alone", dist="uniform"):
    ROWS.append(dict(key=key, n=n, off=off, batch=batch, style=style, dist=dist, expect=expect))


# ---- K16: 15 copies, a key of <= 2^21 points: short up to 2^15 terms, then one fused bucket set with bucket-owning lanes
for n_ in (1, 4095, 4096, P15):
    row("K16", n_, short(n_))
row("K16", 1, short(1), off=P16 - 1)
for n_ in (P15 + 1, P16):
    row("K16", n_, ordinary(n_, 17, 1, 15, 2, FUSED, 4))
for b_, lanes_ in ((2, 32), (3, 16), (8, 16)):
    row("K16", 4096, short(4096, b_), batch=b_)
    row("K16", P15 + 1, ordinary(P15 + 1, 17, 1, 15, 2, FUSED, lanes_, b_), batch=b_)
    row("K16", P16, ordinary(P16, 17, 1, 15, 2, FUSED, lanes_, b_), batch=b_)
row("K16", P15, short(P15), style="inflight")
row("K16", P16, ordinary(P16, 17, 1, 15, 2, FUSED, 16), style="inflight")
# a bucket list of the short path overflows: run again at the finish, alone on the context by then (quads), or term by term below 4096
row("K16", 8192, ordinary(8192, 17, 1, 15, 2, FUSED, 4, path="short_fallback"), dist="overflow")
row("K16", 300, _shape("short_fallback", 300, 1, 15), dist="overflow")
# ---- K22 (one sequence, in this order): the table is not resident at first and the key is too large to build it for 100 terms
row("K22", 100, naive(100))
row("K22", P20 + 1, ordinary(P20 + 1, 17, 3, 5, 0, DIGITS, 32))
row("K22", P21 + 1, ordinary(P21 + 1, 17, 5, 3, 0, DIGITS, 32))
row("K22", P22, ordinary(P22, 17, 5, 3, 0, DIGITS, 32))
row("K22", 100, short(100))                                          # the same call as the first row, now with the 15 copies resident
row("K22", 100, short(100), off=P22 - 100)
row("K22", 5000, short(5000), off=P21 + 17)
row("K22", P20, ordinary(P20, 17, 1, 15, 0, FUSED, 4), off=7)
row("K22", P21, ordinary(P21, 17, 3, 5, 0, DIGITS, 16), style="inflight")
row("K22", P22 - 5, ordinary(P22 - 5, 17, 5, 3, 0, DIGITS, 32), off=5)
# ---- K24: long commitments as 2^20-term pieces, three in flight; the shape is that of the ragged last piece
row("K24", P23 + 100, short(100, pieces=9, piece_terms=P20))
row("K24", P23 + 5000, short(5000, pieces=9, piece_terms=P20))
row("K24", P23 + 40000, ordinary(40000, 17, 1, 15, 2, FUSED, 16, pieces=9, piece_terms=P20))
row("K24", P24 - 3, ordinary(P20 - 3, 17, 1, 15, 0, FUSED, 16, pieces=16, piece_terms=P20), off=3)
# ---- K1COPY: no shifted copies: 13- / 15- / 17-bit windows by length, 20 / 17 / 15 bucket sets through the digit array
row("K1COPY", 4096, ordinary(4096, 13, 20, 1, 2, DIGITS, 32))        # (first: table_copies == 1 and c = 13 — with a larger cap on the table this row would be short)
for n_ in (1, 100, 4095):
    row("K1COPY", n_, naive(n_))
row("K1COPY", 100, naive(100), off=KEYS["K1COPY"] - 100)
for n_ in (5000, P16):
    row("K1COPY", n_, ordinary(n_, 13, 20, 1, 2, DIGITS, 32))
row("K1COPY", P17 - 1, ordinary(P17 - 1, 13, 20, 1, 0, DIGITS, 32))
for n_ in (P17, P18 + 7, P19 - 1):
    row("K1COPY", n_, ordinary(n_, 15, 17, 1, 0, DIGITS, 32))
for n_ in (P19, P20):
    row("K1COPY", n_, ordinary(n_, 17, 15, 1, 0, DIGITS, 32))
row("K1COPY", 5000, ordinary(5000, 13, 20, 1, 2, DIGITS, 32), off=(1 << 25) + 12345)
for b_, lanes_ in ((2, 32), (3, 16), (8, 16)):
    row("K1COPY", 5000, ordinary(5000, 13, 20, 1, 2, DIGITS, lanes_, b_), batch=b_)
    row("K1COPY", P16, ordinary(P16, 13, 20, 1, 2, DIGITS, lanes_, b_), batch=b_)
    row("K1COPY", P18 + 7, ordinary(P18 + 7, 15, 17, 1, 0, DIGITS, lanes_, b_), batch=b_)
row("K1COPY", P16, ordinary(P16, 13, 20, 1, 2, DIGITS, 16), style="inflight")
row("K1COPY", P18 + 7, ordinary(P18 + 7, 15, 17, 1, 0, DIGITS, 16), style="inflight")
row("K1COPY", P19, ordinary(P19, 17, 15, 1, 0, DIGITS, 16), style="inflight")
# without the table a long commitment is cut into passes of 2^24 terms, one at a time, over advancing key ranges
row("K1COPY", KEYS["K1COPY"], ordinary(P22, 17, 15, 1, 0, DIGITS, 32, pieces=3, piece_terms=P24))
row("K1COPY", P24 + 12345, ordinary(12345, 13, 20, 1, 2, DIGITS, 32, pieces=2, piece_terms=P24), off=1000)
DISTRIBUTIONS = ("ones", "minus_one", "witness_like", "small", "top_bits", "zeros", "one_hot")
for n_, e_ in ((5000, ordinary(5000, 13, 20, 1, 2, DIGITS, 32)), (P16, ordinary(P16, 13, 20, 1, 2, DIGITS, 32)),
               (P18 + 7, ordinary(P18 + 7, 15, 17, 1, 0, DIGITS, 32)), (P19, ordinary(P19, 17, 15, 1, 0, DIGITS, 32))):
    for dist_ in DISTRIBUTIONS:
        row("K1COPY", n_, dict(e_), dist=dist_)


def _row_id(r):
    return "%s-n%d-off%d-b%d-%s-%s" % (r["key"], r["n"], r["off"], r["batch"], r["style"], r["dist"])


# ------------------------------------------------------------------------------------------------ the cover of the table (no GPU)
def cover(rows):
    """which shape classes the table reaches: {class name: number of rows}"""
    got = {}

    def hit(name):
        got[name] = got.get(name, 0) + 1
    for r in rows:
        e = r["expect"]
        hit("path " + e["path"])
        if e["window_bits"]:
            hit("c = %d" % e["window_bits"])
            hit("bucket sets %d" % e["bucket_sets"])
            hit("accumulate variant %d" % e["accumulate_variant"])
            hit("pre-phase " + {FUSED: "fused", DIGITS: "digit array"}[e["prephase"]])
            hit("reduction " + {4: "quads", 16: "16 lanes", 32: "32 lanes"}[e["reduce_lanes"]])
            hit("c = %d, %d coarse bins, reduction %s" % (e["window_bits"], e["coarse_bins"], {4: "quads", 16: "16 lanes", 32: "32 lanes"}[e["reduce_lanes"]]))
        if e["pieces"] == 1:
            hit("pieces 1")
        elif e["pieces"] == 2:
            hit("pieces 2")
        elif e["pieces"] > 3 and (r["n"] % e["piece_terms"]) != 0:
            hit("pieces > 3, ragged tail")
        if e["pieces"] > 1 and e["piece_terms"] == P24:
            hit("passes of 2^24 terms over advancing key ranges")
    return got


REQUIRED = (["path naive", "path short", "path short_fallback", "path ordinary"] + ["c = %d" % c for c in (13, 15, 17)] +
            ["bucket sets %d" % s for s in (1, 3, 5, 15, 17, 20)] + ["accumulate variant 0", "accumulate variant 2", "pre-phase fused", "pre-phase digit array",
            "reduction quads", "reduction 16 lanes", "reduction 32 lanes", "pieces 1", "pieces 2", "pieces > 3, ragged tail",
            "passes of 2^24 terms over advancing key ranges"] +
            ["c = %d, %d coarse bins, reduction %s" % (c, WINDOWS_AND_BINS[c][1], k) for c in (13, 15, 17) for k in ("16 lanes", "32 lanes")] +
            ["c = 17, 1024 coarse bins, reduction quads"])


def test_cover_of_the_matrix():
    """every shape class has a row (the first K22 row is the naive path as FIRST choice: 100 terms on a 15-copy key)"""
    got = cover(ROWS)
    missing = [name for name in REQUIRED if not got.get(name)]
    assert not missing, missing
    first = [r for r in ROWS if r["key"] == "K22"][0]
    assert first["expect"]["path"] == "naive" and KEYS["K22"] * 15 * 64 <= 32 << 30
    assert KEYS["K1COPY"] * 15 * 64 > 32 << 30 and [r for r in ROWS if r["key"] == "K1COPY"][0]["expect"]["table_copies"] == 1


def coverage_table():
    """the DESIGN.md table: one line per shape class with the number of rows and the first of them"""
    lines = ["| dispatch shape | rows of `tests/test_gpu_msm_shapes.py` | first row |", "|---|---|---|"]
    first = {}
    for r in ROWS:
        for name in cover([r]):
            first.setdefault(name, _row_id(r))
    got = cover(ROWS)
    for name in REQUIRED:
        lines.append("| %s | %d | `%s` |" % (name, got.get(name, 0), first.get(name, "-")))
    return "\n".join(lines)


def test_design_md_table():
    doc = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert coverage_table() in doc, "DESIGN.md: the table of covered MSM shapes is out of date (python tests/test_gpu_msm_shapes.py prints it)"


# ------------------------------------------------------------------------------------------------ scalars and answers
def _rand_fr(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)          # < 2^252 < r: valid Montgomery residues
    return a


_TABLES = {}


def _table(name):
    if name not in _TABLES:
        _TABLES[name] = ol.fr_vec(list(range(1 << 16))) if name == "below_2pow16" else ol.fr_vec([R_MOD - 1 - x for x in range(1 << 16)])
    return _TABLES[name]


OVERFLOW = sum(3 << (17 * w) for w in range(5)) + sum((7 << 8) << (17 * w) for w in range(6, 11))    # the same digit in several windows (test_gpu_kernels.py)


def scalars(dist, n, seed):
    rng = np.random.default_rng(seed)
    if dist == "uniform":
        s = _rand_fr(n, seed)
        s[::3] = 0
        return s
    if dist == "zeros":
        return np.zeros((n, 4), dtype=np.uint64)
    if dist in ("ones", "minus_one", "overflow"):
        return np.tile(ol.fr_mont({"ones": 1, "minus_one": R_MOD - 1, "overflow": OVERFLOW}[dist]), (n, 1))
    if dist == "one_hot":
        s = np.zeros((n, 4), dtype=np.uint64)
        s[n // 3] = ol.fr_mont(R_MOD - 2)
        return s
    if dist == "small":
        return np.ascontiguousarray(_table("below_2pow16")[rng.integers(0, 4, size=n)])
    if dist == "top_bits":                                           # top window at its maximum, carries everywhere
        return np.ascontiguousarray(_table("top")[rng.integers(0, 1 << 16, size=n)])
    assert dist == "witness_like"                                    # 50 % zero, 25 % below 2^16, 25 % uniform
    s = _rand_fr(n, seed)
    sel = rng.integers(0, 4, size=n)
    s[sel < 2] = 0
    idx = np.nonzero(sel == 2)[0]
    s[idx] = _table("below_2pow16")[rng.integers(0, 1 << 16, size=idx.shape[0])]
    return s


def trapdoor(s, off):
    return ol.g1_mul(ol.g1_generator(), ol.poly_eval(s, 42) * pow(42, off, R_MOD) % R_MOD)


def run_row(ctx, r, seed):
    """the row's commitment(s) in its call style; returns nothing, asserts the shape and then the values"""
    import torch
    import plonkit_amd as pa
    n, off, batch = r["n"], r["off"], r["batch"]
    vecs = [scalars(r["dist"], n, seed + 17 * k) for k in range(batch)]
    dev = [torch.from_numpy(v.view(np.int64)).to("cuda:0") for v in vecs]
    torch.cuda.synchronize()
    if r["style"] == "inflight":                                     # another commitment of the same length is enqueued first and finished first
        other = scalars("uniform", n, seed + 5)
        d_other = torch.from_numpy(other.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        ctx.msm_enqueue_dev(d_other, n, off)
        ctx.msm_enqueue_dev(dev[0], n, off)
        got_other = pa.g1_sum_jacobian(ctx.msm_finish())
        got = [pa.g1_sum_jacobian(ctx.msm_finish())]
    elif batch == 1:
        got_other = None
        got = [ctx.msm_dev(dev[0], n, base_offset=off)]
    else:
        got_other = None
        got = list(ctx.msm_batch_dev(dev, n, base_offset=off))
    shape = ctx.msm_last_shape()
    assert shape == r["expect"], (_row_id(r), {k: (shape[k], r["expect"][k]) for k in FIELDS if shape[k] != r["expect"][k]})
    for k in range(batch):
        assert np.array_equal(np.asarray(got[k]), trapdoor(vecs[k], off)), (_row_id(r), k)
    if got_other is not None:
        assert np.array_equal(got_other, trapdoor(other, off)), (_row_id(r), "the commitment in flight before it")
    if n <= 5000:                                                    # the oracle's own Pippenger over the oracle's own key, shifted by 42^off
        if "crs" not in _TABLES:
            _TABLES["crs"] = ol.crs42(5000)
        if vecs[0].any():
            assert np.array_equal(np.asarray(got[0]), ol.g1_mul(ol.msm(_TABLES["crs"][:n], vecs[0]), pow(42, off, R_MOD))), (_row_id(r), "ol.msm")
        else:
            assert ol.g1_is_inf(np.asarray(got[0])), (_row_id(r), "all-zero scalars")


def _key_ctx(name):
    import plonkit_amd as pa
    c = pa.Context(0)
    c.srs_generate(KEYS[name], 0, 42)
    return c


@pytest.fixture(scope="module")
def k16():
    c = _key_ctx("K16")
    yield c
    c.close()


@pytest.fixture(scope="module")
def k24():
    c = _key_ctx("K24")
    yield c
    c.close()


@pytest.fixture(scope="module")
def k1copy():
    import torch
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info(0)[0]
    c = _key_ctx("K1COPY")
    yield c
    c.synchronize(); torch.cuda.empty_cache()
    print("\nK1COPY: %.2f GiB of device memory held by the key's context after its rows (key, its copy in the accumulation's domain, scratch; buffers only grow)"
          % ((free0 - torch.cuda.mem_get_info(0)[0]) / 2.0 ** 30))
    c.close()


def _rows_of(key):
    return [pytest.param(r, i, id=_row_id(r)) for i, r in enumerate(ROWS) if r["key"] == key]


@pytest.mark.gpu
@pytest.mark.parametrize("r,index", _rows_of("K16"))
def test_shape_then_value_k16(k16, r, index):
    run_row(k16, r, 16000 + index)


@pytest.mark.gpu
def test_shape_then_value_k22_sequence():
    """state-dependent dispatch: the K22 rows in table order on ONE fresh context"""
    ctx = _key_ctx("K22")
    try:
        for i, r in enumerate(ROWS):
            if r["key"] == "K22":
                run_row(ctx, r, 22000 + i)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r,index", _rows_of("K24"))
def test_shape_then_value_k24(k24, r, index):
    run_row(k24, r, 24000 + index)


@pytest.mark.gpu
@pytest.mark.parametrize("r,index", _rows_of("K1COPY"))
def test_shape_then_value_k1copy(k1copy, r, index):
    run_row(k1copy, r, 25000 + index)


@pytest.mark.gpu
def test_msm_differential_fuzz_on_a_one_copy_key():
    """tools/msm_fuzz.py on a key without shifted copies (2^25 + 2^22 points), lengths 1 .. 2^19 + 3 around every window-width and
    variant threshold: random offsets, batch sizes, distributions and call styles against the tau = 42 trapdoor answer"""
    import subprocess
    lengths = [1, 7, 100, 4095, 4096, 4097, 5000, 1 << 13, 12345, 1 << 15, 50000, 1 << 16, (1 << 16) + 1, 100000, (1 << 17) - 3, (1 << 17) - 1, 1 << 17,
               (1 << 18) + 7, (1 << 19) - 1, 1 << 19, (1 << 19) + 3]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "msm_fuzz.py"), "24", "12", str(KEYS["K1COPY"]), ",".join(str(x) for x in lengths)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "mismatches: 0" in r.stdout


if __name__ == "__main__":
    print(coverage_table())
