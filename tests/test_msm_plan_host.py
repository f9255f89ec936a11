"""-m "not gpu": the dispatch of the MSM (plonkit_amd/csrc/msm_plan.h: which kernels, window bits, table copies, pre-phase, accumulate
variant, reduction lanes, pieces and buffer sizes a commitment is given) — tests/host/msm_plan_check.cpp is built as a stand-alone program
with AddressSanitizer and UBSan and run directly (it is not loaded into Python).
  table: the hand-written table of tests/test_gpu_msm_shapes.py (ROWS, KEYS, FIELDS: that module stays the one place where the expected
         shapes are written down) goes to the program row by row, key by key in table order; the program plans every row with the header's
         functions, keeping only the FIFO and the resident table of each key itself (every key starts without a table: no expectation outside
         the K22 sequence depends on the starting state), and its thirteen fields per row must equal `expect` for all rows — without a GPU,
         a 2^24-point key or a key of 2.25 GiB.
  sweep: invariants of the plan over terms x batch x key size x table state x in flight x fused allowed (copies divide 15 and fit the 24-bit
         entry field, windows = 254 / c + 1, at most 1024 coarse bins, nothing truncated to 32 bits, the buffer sizes restated, determinism)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "msm_plan_check.cpp")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_gpu_msm_shapes import FIELDS, KEYS, ROWS, _row_id


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_plan") / "msm_plan_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _clean(r):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_the_header_has_no_hip_include():
    """a stand-alone host program can only check the plan while msm_plan.h and what it includes stay free of the HIP runtime; and the plan
    is a function of its arguments alone: it reads no environment"""
    plan = open(os.path.join(ROOT, "plonkit_amd", "csrc", "msm_plan.h"), encoding="utf-8").read()
    api = open(os.path.join(ROOT, "include", "plonkit_amd.h"), encoding="utf-8").read()
    assert "hip/" not in plan and "hip/" not in api
    assert "getenv" not in plan
    includes = [line.split()[1] for line in plan.splitlines() if line.startswith("#include")]
    assert includes == ["<stdint.h>", "<stddef.h>", '"../../include/plonkit_amd.h"'], includes


def test_every_row_of_the_gpu_table(program):
    keys = list(dict.fromkeys(r["key"] for r in ROWS))
    ordered = [r for k in keys for r in ROWS if r["key"] == k]            # key by key, in table order
    assert len(ordered) == len(ROWS) == 90
    lines = ["%s %d %d %d %s %d" % (r["key"], KEYS[r["key"]], r["n"], r["batch"], r["style"], 1 if r["dist"] == "overflow" else 0) for r in ordered]
    res = subprocess.run([program, "table"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    _clean(res)
    out = res.stdout.split("\n")[:-1]
    assert len(out) == len(ordered), res.stdout[-2000:] + res.stderr[-2000:]
    bad = []
    for r, line in zip(ordered, out):
        cells = line.split()
        assert len(cells) == len(FIELDS), line
        shape = {k: (v if k == "path" else int(v)) for k, v in zip(FIELDS, cells)}
        if shape != r["expect"]:
            bad.append((_row_id(r), {k: (shape[k], r["expect"][k]) for k in FIELDS if shape[k] != r["expect"][k]}))
    assert not bad, bad


def test_sweep_of_the_plan(program):
    res = subprocess.run([program, "sweep"], capture_output=True, text=True, timeout=300)
    _clean(res)
    assert "msm_plan_check: ok" in res.stdout, res.stdout + res.stderr
