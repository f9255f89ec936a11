"""The device pairing check (plonkit_amd/csrc/fq12_dev.h: flat Fq12, sparse line products, the shortened final exponentiation) compiled for
the HOST — its functions are __host__ __device__ — against pairing_product_is_one of pairing.cpp on true pairs, near misses, points at
infinity on either side and a repeated G2 point (tests/host/fq12_dev_check.hip).  No GPU involved: hipcc only compiles."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_device_pairing_code_on_the_host(tmp_path, golden_dir):
    g2 = tmp_path / "g2.bin"
    g2.write_bytes(open(os.path.join(golden_dir, "vk.bin"), "rb").read()[-256:])
    exe = str(tmp_path / "fq12_dev_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "host", "fq12_dev_check.hip"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    r = subprocess.run([exe, str(g2)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "20 cases, 8 are one, 0 mismatches" in r.stdout, r.stdout
