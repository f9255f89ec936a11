"""-m "not gpu": the host half of the R1CS witness check (plonkit_amd/csrc/r1cs_plan.h) — tests/host/r1cs_plan_check.cpp is built as a
stand-alone program with AddressSanitizer and UBSan and run directly (it is not loaded into Python).  The program feeds the plan builder
hand-made R1CS structures (no constraints, one constraint, empty LCs, wire 0, all coefficients distinct / equal / only +-1 / mixed, LC
lengths at long - 1, long, long + 1 and beyond) and checks that every term's (wire, table[coeff_index]) equals its source, that table
entries 0 and 1 are 1 and r - 1, that the offsets are monotone, that every LC is in exactly one work list, and that the plan evaluated
with hostmath.h gives the verdict and the lowest failing constraint of a direct loop over R1cs::lc."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "r1cs_plan_check.cpp")


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("r1cs_plan") / "r1cs_plan_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_header_has_no_hip_include():
    """a stand-alone host program can only check the plan while r1cs_plan.h and what it includes stay free of the HIP runtime"""
    csrc = os.path.join(ROOT, "plonkit_amd", "csrc")
    for name in ("r1cs_plan.h", "circuit.h", "hostmath.h"):
        assert "hip/" not in open(os.path.join(csrc, name), encoding="utf-8").read(), name


def test_plan_against_the_direct_loop(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "r1cs_plan_check: ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
