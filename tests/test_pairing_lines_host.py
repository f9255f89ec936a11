"""The line table of the Miller loop (plonkit_amd/csrc/pairing.cpp miller_lines — what plk_vk_load builds on the host and uploads):
tests/host/pairing_lines_check.cpp evaluates the loop from the table and compares it with miller_loop coefficient for coefficient, for the
two points of plk_crs42_g2_bytes and the G2 section of the golden vk.bin, at G1 = infinity and at i * G, i = 1..10.  No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_miller_loop_from_the_line_table(tmp_path, golden_dir):
    import plonkit_amd as pa
    crs = tmp_path / "crs42_g2.bin"
    crs.write_bytes(pa.crs42_g2_bytes())
    vk = tmp_path / "vk_g2.bin"
    vk.write_bytes(open(os.path.join(golden_dir, "vk.bin"), "rb").read()[-256:])
    exe = str(tmp_path / "pairing_lines_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "host", "pairing_lines_check.cpp"), "-o", exe])
    r = subprocess.run([exe, str(crs), str(vk)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "45 checks, 0 mismatches" in r.stdout, r.stdout
