"""-m "not gpu": the dispatch of the scalar NTT (plonkit_amd/csrc/ntt_dispatch.h: digits, tile, and per pass the kernel, its geometry, scalings, buffers,
grid, LDS bytes and inter-pass twiddle table; the batching rules of the four callers; the eviction of twiddle tables) — tests/host/ntt_dispatch_check.cpp is
built as a stand-alone program with AddressSanitizer and UBSan and run directly (it is not loaded into Python).
  table:    the size -> passes table of DESIGN.md §4.3, written out by hand below (TABLE), reproduced row by row for plain, inverse and coset transforms and
            for the zero-padded extension (nonzero = n/4, 4n = 2^5 .. 2^28); which pass wants a twiddle table, and which has 1/n folded in.
  sweep:    invariants of the plan over log_n x count x direction x nonzero x input scaling x output scaling x tables allowed — among them the closed trap:
            a barrier pass never gets more than 2^11 elements or more LDS than its kernel's attribute (the 2^21 plan with a barrier first pass did).
  batch:    the four batching rules restated for log_n 1..28 and counts 1..18.
  eviction: hand-made table sets for each outcome.
  coverage: the NTT size lists of tests/test_gpu_kernels.py and tests/test_gpu_large.py, run through the plan, reach every kernel instantiation the
            dispatcher can name — the docstrings' "cover every pass shape" as a check."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ntt_dispatch_check.cpp")
HEADER = os.path.join(ROOT, "plonkit_amd", "csrc", "ntt_dispatch.h")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_gpu_kernels as gk
from tests import test_gpu_large as gl

NONE, TWO_LEVEL, PER_ELEMENT = 0, 1, 2
FIELDS = ("role family row_bits log_tile log_r log_c log_inner log_r1 log_m1 log_m2 nonzero quarter pre post reads writes grid_x block lds_bytes "
          "wants_table table_bits table_key table_scaled").split()
COLS, ROWS = 0, 1
BARRIER, WAVE = 0, 1
W_LDS, W_LDS_BIG = 36 * 8 * (4 * 68 + 8), 36 * 16 * (4 * 68 + 8)          # 80 640 and 161 280 B
LDS_ROWS, LDS_COLS = 36 << 11, 96 * 1024

# The parent's dispatch, by hand: log_n -> (digits, passes); a pass is (role, family, row bits, log_c), W on the 2048-element tile unless a fifth entry
# names the tile.  W = ntt_pass_w, B = ntt_pass_cols / ntt_pass_rows.
TABLE = {n: ((n,), [(ROWS, BARRIER, n, 0)]) for n in range(1, 12)}
TABLE.update({
    12: ((6, 6), [(COLS, BARRIER, 6, 5), (ROWS, BARRIER, 6, 5)]),
    13: ((7, 6), [(COLS, WAVE, 7, 4), (ROWS, BARRIER, 6, 5)]),
    14: ((7, 7), [(COLS, WAVE, 7, 4), (ROWS, WAVE, 7, 4)]),
    15: ((8, 7), [(COLS, WAVE, 8, 3), (ROWS, WAVE, 7, 4)]),
    16: ((8, 8), [(COLS, WAVE, 8, 3), (ROWS, WAVE, 8, 3)]),
    17: ((9, 8), [(COLS, WAVE, 9, 2), (ROWS, WAVE, 8, 3)]),
    18: ((9, 9), [(COLS, WAVE, 9, 2), (ROWS, WAVE, 9, 2)]),
    19: ((10, 9), [(COLS, WAVE, 10, 1), (ROWS, WAVE, 9, 2)]),
    20: ((10, 10), [(COLS, WAVE, 10, 1), (ROWS, WAVE, 10, 1)]),
    21: ((11, 10), [(COLS, WAVE, 11, 1, 12), (ROWS, WAVE, 10, 2, 12)]),
    22: ((8, 7, 7), [(COLS, WAVE, 8, 3), (COLS, WAVE, 7, 4), (ROWS, WAVE, 7, 4)]),
    23: ((9, 7, 7), [(COLS, WAVE, 9, 2), (COLS, WAVE, 7, 4), (ROWS, WAVE, 7, 4)]),
    24: ((8, 8, 8), [(COLS, WAVE, 8, 3), (COLS, WAVE, 8, 3), (ROWS, WAVE, 8, 3)]),
    25: ((9, 8, 8), [(COLS, WAVE, 9, 2), (COLS, WAVE, 8, 3), (ROWS, WAVE, 8, 3)]),
    26: ((9, 9, 8), [(COLS, WAVE, 9, 2), (COLS, WAVE, 9, 2), (ROWS, WAVE, 8, 3)]),
    27: ((9, 9, 9), [(COLS, WAVE, 9, 2), (COLS, WAVE, 9, 2), (ROWS, WAVE, 9, 2)]),
    28: ((10, 9, 9), [(COLS, WAVE, 10, 1), (COLS, WAVE, 9, 2), (ROWS, WAVE, 9, 2)]),
})
# the twelve kernels ntt.hip builds, as the program names them
KERNELS = {"cols B", "rows B"} | {"%s W<%d>" % (r, b) for r in ("cols", "rows") for b in (7, 8, 9, 10)} | {"cols W<11, 12>", "rows W<10, 12>"}


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ntt_dispatch") / "ntt_dispatch_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(program, mode, lines=()):
    r = subprocess.run([program, mode], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout.split("\n")[:-1]


def _plans(program, inputs):
    """inputs: (log_n, count, inverse, nonzero, pre, post, tables) -> one dict per input: passes, log_tile, scratch, digits, pass (a list of field dicts)"""
    out = iter(_run(program, "plan", ["%d %d %d %d %d %d %d" % i for i in inputs]))
    plans = []
    for _ in inputs:
        head = [int(x) for x in next(out).split()]
        p = {"passes": head[0], "log_tile": head[1], "scratch": head[2], "digits": tuple(d for d in head[3:] if d), "pass": []}
        for _ in range(p["passes"]):
            cells = [int(x) for x in next(out).split()]
            assert len(cells) == len(FIELDS)
            p["pass"].append(dict(zip(FIELDS, cells)))
        plans.append(p)
    assert next(out, None) is None
    return plans


def test_the_header_is_host_only():
    """a stand-alone host program can only check the plan while ntt_dispatch.h and what it includes stay free of the HIP runtime; and the plan is a function
    of its arguments alone: it reads no environment"""
    plan = open(HEADER, encoding="utf-8").read()
    tile = open(os.path.join(ROOT, "plonkit_amd", "csrc", "ntt_plan.h"), encoding="utf-8").read()
    assert "hip/" not in plan and "hip/" not in tile
    assert "getenv" not in plan and "getenv" not in tile
    includes = [line.split()[1] for line in plan.splitlines() if line.startswith("#include")]
    assert includes == ["<stdint.h>", "<stddef.h>", '"ntt_plan.h"'], includes
    assert [line.split()[1] for line in tile.splitlines() if line.startswith("#include")] == ["<stdint.h>"]


def _expect_pass(log_n, row, index, passes):
    role, family, bits, log_c = row[:4]
    tile = row[4] if len(row) > 4 else 11
    digits = TABLE[log_n][0]
    e = {"role": role, "family": family, "log_r": bits, "log_c": log_c, "grid_x": (1 << log_n) >> (bits + log_c)}
    if family == WAVE:
        e.update(row_bits=bits, log_tile=tile, block=512 if tile == 11 else 1024, lds_bytes=W_LDS if tile == 11 else W_LDS_BIG)
    else:
        e.update(row_bits=0, log_tile=0, block=512, lds_bytes=36 << (bits + log_c))
    if role == COLS:
        e.update(log_inner=log_n - sum(digits[:index + 1]), log_r1=0, log_m1=0, log_m2=0)
    else:
        e.update(log_inner=0, log_r1=digits[0] if passes > 1 else 0, log_m1=digits[1] if passes > 2 else 0, log_m2=0)
    e.update(reads=0 if index == 0 else 1, writes=2 if index == passes - 1 else 1)
    return e


@pytest.mark.parametrize("kind", ["plain", "inverse", "coset", "inverse coset", "padded"])
def test_every_row_of_the_table(program, kind):
    """`padded`: the extension by 4 (lde4_batch_dev), nonzero = n/4 for 4n = 2^5 .. 2^28 — the same kernels; `quarter` at 2^12 alone"""
    inverse = kind.startswith("inverse")
    pre = TWO_LEVEL if kind in ("coset", "padded") else NONE
    post = TWO_LEVEL if kind == "inverse coset" else NONE
    sizes = [n for n in sorted(TABLE) if kind != "padded" or n >= 5]
    assert sorted(TABLE) == list(range(1, 29))
    inputs = [(n, 1, int(inverse), (1 << n) >> 2 if kind == "padded" else 0, pre, post, 1) for n in sizes]
    bad = []
    for n, plan in zip(sizes, _plans(program, inputs)):
        digits, rows = TABLE[n]
        if plan["digits"] != digits or plan["passes"] != len(rows) or plan["log_tile"] != (12 if n == 21 else 11):
            bad.append((n, plan["digits"], plan["passes"], plan["log_tile"]))
            continue
        if plan["scratch"] != (32 << n if len(rows) > 1 else 0):
            bad.append((n, "scratch", plan["scratch"]))
        for i, (row, got) in enumerate(zip(rows, plan["pass"])):
            e = _expect_pass(n, row, i, len(rows))
            first, last = i == 0, i == len(rows) - 1
            e.update(nonzero=(1 << n) >> 2 if first and kind == "padded" else 0, quarter=1 if kind == "padded" and n == 12 and first else 0,
                     pre=pre if first else NONE, post=post if last else NONE)
            # twiddle tables: the first pass of 2^15 .. 2^25 (1/n folded in on inverse transforms), the second pass of 2^24 .. 2^28; the first pass of
            # 2^26 .. 2^28 composes, and so does every sub-transform of at most 2^14 points
            wants = (i == 0 and len(rows) > 1 and 15 <= n <= 25) or (i == 1 and len(rows) == 3 and 24 <= n <= 28)
            e.update(wants_table=int(wants), table_bits=(n - sum(digits[:i])) if wants else 0, table_scaled=int(wants and inverse and first))
            diff = {k: (got[k], v) for k, v in e.items() if got[k] != v}
            if not wants and got["table_key"]:
                diff["table_key"] = (got["table_key"], 0)
            if diff:
                bad.append((n, i, diff))
    assert not bad, bad


def test_without_tables_no_pass_wants_one(program):
    for plan in _plans(program, [(n, 1, inv, 0, NONE, NONE, 0) for n in range(1, 29) for inv in (0, 1)]):
        assert all(not q["wants_table"] for q in plan["pass"])


def test_the_big_tile_needs_two_wave_passes(program):
    """the latent launch failure: a 2^21 transform whose first pass is zero-padded AND reads a per-element input table is not the wave kernel's; it used to be
    launched as ntt_pass_cols with 36 * 2^12 = 147 456 B of LDS (attribute: 96 KiB) and 2^12 elements for 512 threads.  It is 7 + 7 + 7 on the small tile now."""
    plan, = _plans(program, [(21, 4, 0, 1 << 19, PER_ELEMENT, NONE, 1)])
    assert plan["digits"] == (7, 7, 7) and plan["log_tile"] == 11 and plan["scratch"] == 4 * 32 << 21
    first, mid, last = plan["pass"]
    assert (first["family"], first["log_r"], first["log_c"], first["lds_bytes"], first["block"]) == (BARRIER, 7, 4, 36 << 11, 512)
    assert first["lds_bytes"] <= LDS_COLS
    assert (mid["family"], mid["row_bits"], last["family"], last["row_bits"]) == (WAVE, 7, WAVE, 7)
    # and with either of the two alone it stays 11 + 10
    for nonzero, pre in ((1 << 19, TWO_LEVEL), (0, PER_ELEMENT)):
        plan, = _plans(program, [(21, 4, 0, nonzero, pre, NONE, 1)])
        assert plan["digits"] == (11, 10) and plan["log_tile"] == 12 and all(q["family"] == WAVE for q in plan["pass"])


def test_sweep_of_the_plan(program):
    out = _run(program, "sweep")
    assert out and out[-1].startswith("ntt_dispatch_check: ok"), out


def test_batch_plan(program):
    """transforms (polynomials for the two extensions) per launch, the four callers' rules restated: the launches cover the count, none exceeds 16 transforms,
    and none of the three bounded rules that holds more than one item exceeds 2 GiB of ping-pong scratch (count x n x 32 B)"""
    PLAIN, LDE4, LDE4CM, PROVER = range(4)
    per = {}
    for line in _run(program, "batch"):
        rule, log_n, p = (int(x) for x in line.split())
        per[rule, log_n] = p
    assert len(per) == 4 * 28
    for log_n in range(1, 29):
        want = {PLAIN: 16,
                LDE4: 16 if log_n + 2 <= 22 else (4 if log_n + 2 <= 24 else 1),
                LDE4CM: max([q for q in (4, 3, 2) if q * 4 * 32 << log_n <= 2 << 30], default=1),
                PROVER: 4 if log_n <= 22 else 1}
        for rule in range(4):
            p = per[rule, log_n]
            assert p == want[rule], (rule, log_n, p)
            transforms = p * (4 if rule == LDE4CM else 1)
            points = log_n + 2 if rule == LDE4 else log_n
            assert 1 <= transforms <= 16
            if rule != PLAIN:                                # (ntt_batch_dev takes what its caller hands it, sixteen at a time: it has no scratch bound)
                assert p == 1 or transforms * 32 << points <= 2 << 30, (rule, log_n)
            for count in range(1, 19):
                launches = [min(p, count - done) for done in range(0, count, p)]
                assert sum(launches) == count and all(1 <= b <= p for b in launches)


def test_eviction(program):
    """(clock, want, cap, tables as (key, bytes, last use)) -> the keys that go, oldest idle first, or "compose".  A table is idle when it has not been asked
    for during the last 96 requests: last use + 96 < clock."""
    MB = 1 << 20
    cases = [
        # a fit: nothing goes, idle tables or not
        ((500, 32 * MB, 128 * MB, [(1, 32 * MB, 1), (2, 32 * MB, 499)]), "drop"),
        ((1, 32 * MB, 32 * MB, []), "drop"),
        # the oldest idle tables, and only as many as it takes: one of three here ...
        ((500, 32 * MB, 96 * MB, [(7, 32 * MB, 20), (5, 32 * MB, 10), (9, 32 * MB, 30)]), "drop 5"),
        # ... two for a table twice the size, in order of age, whatever their order in the set ...
        ((500, 64 * MB, 96 * MB, [(7, 32 * MB, 20), (9, 32 * MB, 30), (5, 32 * MB, 10)]), "drop 5 7"),
        # ... and a large old one frees enough by itself
        ((500, 64 * MB, 128 * MB, [(3, 96 * MB, 5), (4, 16 * MB, 6), (6, 16 * MB, 499)]), "drop 3"),
        # tables asked for within the last 96 requests are never chosen: 404 + 96 = 500 is not idle at clock 500, 403 is
        ((500, 32 * MB, 64 * MB, [(1, 32 * MB, 404), (2, 32 * MB, 403)]), "drop 2"),
        ((500, 32 * MB, 64 * MB, [(1, 32 * MB, 404), (2, 32 * MB, 450)]), "compose"),
        # the idle ones do not free enough beside the tables in use: nothing goes, the pass composes
        ((500, 64 * MB, 96 * MB, [(1, 32 * MB, 10), (2, 32 * MB, 480), (3, 32 * MB, 490)]), "compose"),
        # a table larger than the cap composes, and drops nothing on the way
        ((500, 128 * MB, 64 * MB, [(1, 32 * MB, 10)]), "compose"),
        # the sequence of the GPU test (64 MB cap): 2^20 forward + inverse resident, a 2^21 table composes while they are young and replaces both once idle
        ((3, 64 * MB, 64 * MB, [(0x0a0a, 32 * MB, 4), (0x80140a0a, 32 * MB, 2)]), "compose"),
        ((103, 64 * MB, 64 * MB, [(0x0a0a, 32 * MB, 4), (0x80140a0a, 32 * MB, 2)]), "drop %d %d" % (0x80140a0a, 0x0a0a)),
    ]
    lines = ["%d %d %d %d %s" % (clock, want, cap, len(tabs), " ".join("%d %d %d" % t for t in tabs)) for (clock, want, cap, tabs), _ in cases]
    out = _run(program, "evict", lines)
    assert len(out) == len(cases)
    for ((clock, want, cap, tabs), expect), got in zip(cases, out):
        assert got.strip() == expect, (clock, want, cap, tabs, got)


def test_the_gpu_sizes_reach_every_kernel(program):
    """every (role, family, row bits, tile) any plan names has a GPU test size that launches it: the entry points the size lists of tests/test_gpu_kernels.py
    and tests/test_gpu_large.py run, through the plan.  A thirteenth instantiation without a size fails here."""
    reachable = set(_run(program, "reachable"))
    assert reachable == KERNELS, reachable ^ KERNELS
    runs = []
    for n in gk.NTT_ORACLE_LOG_N + gk.NTT_LARGE_PROPERTIES_LOG_N + gl.NTT_TWO_ADICITY_LOG_N + gl.NTT_WORST_CASE_LOG_N + gl.NTT_RECURSIVE_LOG_N:
        runs += [("ntt", n, 1), ("intt", n, 1)]
    for n in gk.NTT_EXTREME_LOG_N:
        runs += [("ntt", n, 1), ("intt", n, 1), ("coset", n, 1)]
    for n in gk.NTT_COSET_LOG_N:
        runs += [("coset", n, 1), ("icoset", n, 1)]
    runs += [("lde4", n, 1) for n in gk.LDE4_LOG_N]
    for n, count in gk.LDE4CM_SHAPES:
        runs += [("lde4cm", n, count)] + ([("lde4", n, 1)] if n > 16 else [])
    for n in gk.ICOSET4CM_LOG_N:
        runs += [("coset", n + 2, 1), ("icoset4cm", n, 1)]
    out = _run(program, "kernels", ["%s %d %d" % r for r in runs])
    assert len(out) == len(runs)
    reached = set()
    for line in out:
        reached |= set(line.split("; "))
    assert reached == reachable, reachable - reached
