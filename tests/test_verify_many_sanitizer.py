"""AddressSanitizer + UndefinedBehaviorSanitizer over the host half of plk_verify_many as a stand-alone program (tests/host/sanitize_verify_many.cpp,
its own main, no preloaded runtime): plk_verify_terms and the Miller line-table builder on the golden files, every truncation of the proof and a
proof of the wrong input count.  No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_verify_terms_and_line_tables_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_verify_many")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "host", "sanitize_verify_many.cpp"), "-o", exe])
    r = subprocess.run([exe, os.path.join(GOLD, "vk.bin"), os.path.join(GOLD, "proof.bin")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout + r.stderr)[-4000:]
