"""-m "not gpu": the host half of the one-pass openings (plonkit_amd/csrc/kzg_all_plan.h) — tests/host/kzg_all_plan_check.cpp is built as a
stand-alone program with AddressSanitizer and UBSan and run directly (it is not loaded into Python).  The program holds the two views of
each arrangement against each other (where coefficient i / key point j lands, what stands at position m), checks the limits (2^25 accepted,
2^26 refused; a key of N - 2 points refused, N - 1 and N accepted) and the scratch layout, and prints both index maps for log_n = 0 .. 12;
this file compares the printed maps with the Python-integer model of tests/gen/fk20_cases.py, whose correlation tests/test_fk20_cases_host.py
holds against the definition of an opening."""
import os
import shutil
import subprocess

import pytest

from tests.gen import fk20_cases as fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "kzg_all_plan_check.cpp")
HEADER = os.path.join(ROOT, "plonkit_amd", "csrc", "kzg_all_plan.h")


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kzg_all_plan") / "kzg_all_plan_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return r.stdout


def test_the_header_has_no_hip_include():
    """a stand-alone host program can only check the plan while kzg_all_plan.h stays free of the HIP runtime"""
    text = open(HEADER, encoding="utf-8").read()
    assert "hip/" not in text and '#include "' not in text


def test_limits_views_and_layout(output):
    assert "kzg_all_plan_check: ok" in output


def test_the_index_maps_are_the_models(output):
    maps = {}
    for line in output.splitlines():
        if line[:2] in ("C ", "T "):
            words = line.split()
            maps[(words[0], int(words[1]))] = [None if w == "-1" else int(w) for w in words[2:]]
    for log_n in range(13):
        assert maps[("C", log_n)] == fk.c_sources(log_n), log_n
        assert maps[("T", log_n)] == fk.t_sources(log_n), log_n
        assert maps[("T", log_n)] != fk.t_sources(log_n, wrong="t_swapped") or log_n <= 1, log_n
