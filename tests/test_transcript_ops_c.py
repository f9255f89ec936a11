"""tests/host/transcript_ops.c: a C program hands a transcript of its own to the library as a plk_transcript_ops table (include/plonkit_amd.h).
Its host half (plk_verify_with, plk_verify_terms_with on the golden pair) runs without a GPU, once against the built library and once as a
stand-alone AddressSanitizer + UndefinedBehaviorSanitizer build of the host sources; its GPU half (plk_prove_witness under the table, then
plk_verify_many_with with PLK_TRANSCRIPT_CONCURRENT) runs with -m gpu."""
import os
import shutil
import subprocess

import pytest

import plonkit_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "transcript_ops.c")
C_FLAGS = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
pytestmark = pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not on PATH")


def _build(tmp_path):
    exe = str(tmp_path / "transcript_ops")
    libdir = os.path.dirname(pa.lib_path())
    subprocess.check_call(["gcc", "-O2"] + C_FLAGS + [SRC, "-o", exe, "-L", libdir, "-lplonkit_amd", "-Wl,-rpath," + libdir])
    return exe


def _golden(golden_dir):
    return [os.path.join(golden_dir, "vk.bin"), os.path.join(golden_dir, "proof.bin")]


def test_host_half_against_the_library(tmp_path, golden_dir):
    r = subprocess.run([_build(tmp_path), "host"] + _golden(golden_dir), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK" and int(r.stdout.split()[1]) >= 20, r.stdout + r.stderr


def test_host_half_under_the_sanitizers(tmp_path, golden_dir):
    """the C program and the host sources, both instrumented, in one stand-alone executable"""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, exe = str(tmp_path / "transcript_ops.o"), str(tmp_path / "transcript_ops_san")
    subprocess.check_call(["gcc"] + san + C_FLAGS + ["-DTRANSCRIPT_OPS_HOST_ONLY", "-c", SRC, "-o", obj])
    subprocess.check_call(["g++", "-std=c++17", "-pthread"] + san + [os.path.join(ROOT, "tests", "host", "sanitize_transcript_ops.cpp"), obj, "-o", exe])
    r = subprocess.run([exe, "host"] + _golden(golden_dir), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr


@pytest.mark.gpu
def test_gpu_half_through_the_c_abi_alone(tmp_path):
    r = subprocess.run(["timeout", "-k", "10", "120", _build(tmp_path), "gpu"], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", r.stdout + r.stderr
