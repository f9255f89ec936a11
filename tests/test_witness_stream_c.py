"""tests/host/witness_stream.c: a C program (include/plonkit_amd.h, no Python in the proving process) makes one setup and proves three
.wtns byte strings through plk_prove_wtns.  It compiles as C99 against the header wherever the library has been built (-m "not gpu") and
runs on the GPU (-m gpu)."""
import os
import shutil
import subprocess

import pytest

import plonkit_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "witness_stream")
    libdir = os.path.dirname(pa.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "witness_stream.c"), "-o", exe, "-L", libdir, "-lplonkit_amd", "-Wl,-rpath," + libdir])
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not on PATH")
def test_witness_stream_compiles_against_the_header(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not on PATH")
def test_witness_stream_through_the_c_abi_alone(tmp_path):
    r = subprocess.run(["timeout", "-k", "10", "120", _build(tmp_path), "12"], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and r.stdout.split() == ["OK", "3"], r.stdout + r.stderr
