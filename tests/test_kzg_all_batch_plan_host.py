"""-m "not gpu": the host half of the batched one-pass openings (the batch functions of plonkit_amd/csrc/kzg_all_plan.h) —
tests/host/kzg_all_batch_plan_check.cpp is built as a stand-alone program with AddressSanitizer and UBSan and run directly (it is not loaded
into Python).  The program checks the limit of a launch (exactly 2^26 points accepted, one polynomial more refused, the byte arithmetic at the
limit in size_t), the scratch regions (disjoint, 16-byte aligned, fk_scratch for a batch of one), the map from a flattened butterfly to
(polynomial, butterfly) as a bijection for log_n = 1 .. 9 and counts 1, 3, 37, that both points of every butterfly lie inside the polynomial's
own stride block at stride N and 2N, and that the output gather reads only the first N of each block."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "kzg_all_batch_plan_check.cpp")


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


def test_limit_scratch_butterflies_and_gather(tmp_path):
    exe = str(tmp_path / "kzg_all_batch_plan_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    assert "kzg_all_batch_plan_check: ok" in r.stdout
