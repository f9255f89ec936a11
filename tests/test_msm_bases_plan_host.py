"""-m "not gpu": the plan of a commitment against caller-supplied bases (plonkit_amd/csrc/msm_plan.h: msm_plan_bases_pass,
msm_plan_bases_call) — tests/host/msm_bases_plan_check.cpp is built as a stand-alone program with AddressSanitizer and UBSan and run directly
(it is not loaded into Python).
  table: the shapes plk_msm_last_shape reports after plk_msm_g1_bases*, written down here by hand (EXPECT_ROWS; tests/test_gpu_msm_bases.py
         asserts the same function of n and batch on the GPU): no key, so ONE copy and the window widths of a key without shifted copies.
  sweep: copies == 1, groups == windows == 254 / c + 1, at most 1024 coarse bins, nothing truncated to 32 bits, table_request == 0,
         determinism, the pass plan equals msm_plan_pipeline(terms, batch, terms, 1, pick_window_bits(terms, false), msm_index_bits(terms),
         false, fused_allowed), and the call plan is ceil(terms / 2^24) passes, at least one, one at a time."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "msm_bases_plan_check.cpp")

FIELDS = ("path", "batch", "table_copies", "window_bits", "windows", "bucket_sets", "fine_bits", "coarse_bins", "accumulate_variant", "prephase",
          "reduce_lanes", "pieces", "piece_terms")
TERMS = (0, 1, 4095, 4096, 1 << 16, (1 << 16) + 1, (1 << 17) - 1, 1 << 17, (1 << 19) - 1, 1 << 19, 1 << 24)
BATCHES = (1, 2, 3, 8)


def expected_shape(n, batch):
    """the shape of one pass of `n` terms and `batch` scalar vectors against caller-supplied bases"""
    e = dict.fromkeys(FIELDS, 0)
    e.update(batch=batch, pieces=1, piece_terms=n)
    if n == 0:
        e["path"] = "empty"
    elif n < 4096:
        e.update(path="naive", table_copies=1)
    else:
        c, windows, bins = (13, 20, 64) if n < 1 << 17 else (15, 17, 256) if n < 1 << 19 else (17, 15, 1024)
        e.update(path="ordinary", table_copies=1, window_bits=c, windows=windows, bucket_sets=windows, fine_bits=6, coarse_bins=bins,
                 accumulate_variant=2 if n <= 1 << 16 else 0, prephase=2, reduce_lanes=32 if batch <= 2 else 16)
    return e


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_bases_plan") / "msm_bases_plan_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _clean(r):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_table_of_shapes(program):
    rows = [(n, b) for n in TERMS for b in BATCHES]
    res = subprocess.run([program, "table"], input="".join("%d %d\n" % r for r in rows), capture_output=True, text=True, timeout=300)
    _clean(res)
    out = res.stdout.split("\n")[:-1]
    assert len(out) == len(rows) == 44, res.stdout[-2000:] + res.stderr[-2000:]
    bad = []
    for (n, b), line in zip(rows, out):
        cells = line.split()
        assert len(cells) == len(FIELDS), line
        shape = {k: (v if k == "path" else int(v)) for k, v in zip(FIELDS, cells)}
        want = expected_shape(n, b)
        if shape != want:
            bad.append((n, b, {k: (shape[k], want[k]) for k in FIELDS if shape[k] != want[k]}))
    assert not bad, bad


def test_sweep_of_the_plan(program):
    res = subprocess.run([program, "sweep"], capture_output=True, text=True, timeout=300)
    _clean(res)
    assert "msm_bases_plan_check: ok" in res.stdout, res.stdout + res.stderr
