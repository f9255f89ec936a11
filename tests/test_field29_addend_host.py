"""The products with a folded addend (plonkit_amd/csrc/field29_dev.h: mulw2_add) and the mixed addition of msm_accumulate's plain kernel
built on them (ec29_dev.h: xyzzw_add_mixed_flag) compiled for the HOST and compared with the forms they replace (tests/host/
field29_addend_check.hip): bit for bit for the products, on random operands and at the documented limb and value bounds, with a 128-bit
shadow of the 64-bit column accumulators; the addition against a reference copy of the earlier one on more than 10^5 random and edge
operands (P = +-Q, accumulator at the identity, y negated).  No GPU involved (hipcc only compiles)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_addend_products_and_mixed_addition_against_the_forms_they_replace(tmp_path):
    exe = str(tmp_path / "field29_addend_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "plonkit_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "field29_addend_check.hip"), "-o", exe], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert "addend forms: 0 mismatches" in r.stdout, r.stdout
    m = re.search(r"mixed addition: 0 mismatches in (\d+) cases", r.stdout)
    assert m and int(m.group(1)) >= 100000, r.stdout
