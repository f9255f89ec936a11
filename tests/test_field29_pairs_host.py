"""The work-priced forms of the kernels around msm_accumulate compiled for the HOST and compared with the forms they stand in for
(tests/host/field29_pairs_check.hip): xyzzw_add_pairs (ec29_dev.h, the full addition of the work-bound bucket reduction) against xyzzw_add in
all 36 limbs on more than 10^5 pairs of lazily reduced operands, edge cases included, with a 128-bit shadow of every 64-bit column chain;
fr_canonical_w and recode17_w (field29_dev.h, msm_shape.h: the scalar recoding on the 29-bit layer) against to_canonical and recode17 on the
edge scalars and more than 10^5 random ones.  No GPU involved (hipcc only compiles)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_pairs_addition_and_limb_recoding_against_the_forms_they_stand_in_for(tmp_path):
    exe = str(tmp_path / "field29_pairs_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "plonkit_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "field29_pairs_check.hip"), "-o", exe], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    m = re.search(r"full addition: 0 mismatches in (\d+) cases \((\d+) on the hot path, (\d+) doublings in other coordinates, (\d+) P - P\)", r.stdout)
    assert m and int(m.group(1)) >= 100000 and int(m.group(2)) >= 50000 and int(m.group(3)) >= 100 and int(m.group(4)) >= 100, r.stdout
    m = re.search(r"scalars: 0 mismatches in (\d+) cases", r.stdout)
    assert m and int(m.group(1)) >= 100000, r.stdout
