"""-m "not gpu": the working memory of the batch verifiers (plonkit_amd/csrc/vm_arena.h) — tests/host/vm_arena_check.cpp is built as a
stand-alone program with AddressSanitizer and UBSan and run directly (it is not loaded into Python).  The program walks m in {1, 15, 16, 17,
65535, 65536}, every combination of the optional parts (none / key indices / offsets and raw bytes / all three) and raw byte counts 0, 1, 15
and 16: order, 16-byte alignment, no overlap, the end within bytes, bytes monotone in m, and the seven fixed parts where the hand-carved
arena of the packed calls had them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "vm_arena_check.cpp")
HEADER = os.path.join(ROOT, "plonkit_amd", "csrc", "vm_arena.h")


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


def test_the_header_has_no_hip_include():
    text = open(HEADER, encoding="utf-8").read()
    assert "hip/" not in text and '#include "' not in text


def test_the_layout_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "vm_arena_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    assert r.stdout.splitlines()[-1] == "vm_arena_check: ok (60 shapes)"
