"""The host side of a key set (plonkit_amd/csrc/vkset_plan.h: which keys share a line table, the layout of the device image, the validation
of a key-index array, the compaction of (proof, key) pairs) and the __host__ __device__ lookup every lane of the mixed kernels goes through
(vkset_dev.h), run by the stand-alone program tests/host/verify_mixed_check.hip: its own main, compiled for the HOST, nothing loaded into
Python.  It also runs the front lane code per key THROUGH the lookup against verify_terms_parsed, for the keys A and F of
tests/gen/mixed_keys.py (they differ in n only).  Built once plainly and once with host AddressSanitizer + UndefinedBehaviorSanitizer; every
image and every proof sits in a heap block of exactly its own length.  No GPU involved."""
import os
import re
import shutil
import subprocess

import pytest

from tests.gen import mixed_keys as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "verify_mixed_check.hip")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the check program twice, compiled side by side: plain, and host code only with the host sanitizers (no device code, GPU sanitizing off)"""
    d = tmp_path_factory.mktemp("verify_mixed")
    plain, san = str(d / "verify_mixed_check"), str(d / "verify_mixed_check_san")
    jobs = [subprocess.Popen(["hipcc", "--offload-host-only", "-O2", "-std=c++17", SRC, "-o", plain], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(["hipcc", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17",
                              SRC, "-o", san], stderr=subprocess.PIPE, text=True)]
    errs = [j.communicate()[1] for j in jobs]
    assert jobs[0].returncode == 0, errs[0][-4000:]
    return plain, (san if jobs[1].returncode == 0 else None), errs[1]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """vk A, vk F, the proof forged for A, the proof forged for F"""
    d = tmp_path_factory.mktemp("verify_mixed_cases")
    a, f = mk.forged("A"), mk.forged("F")
    assert a.valid and f.valid and a.vk != f.vk and a.vk[-256:] == f.vk[-256:]
    assert sum(x != y for x, y in zip(a.vk, f.vk)) == 1                  # one byte of the key: n
    out = []
    for name, data in (("A.vk.bin", a.vk), ("F.vk.bin", f.vk), ("A.proof.bin", a.proof), ("F.proof.bin", f.proof)):
        p = d / name
        p.write_bytes(data)
        out.append(str(p))
    return out


def _judge(out):
    assert "0 mismatches" in out, out[-4000:]
    m = re.search(r"^(\d+) checks$", out, re.M)
    assert m and int(m.group(1)) >= 1000, out[-2000:]
    assert "front: 3 (proof, key) pairs go on, 3 are settled by the front end" in out, out[-2000:]


def test_key_set_plan_and_lookup_on_the_host(programs, files):
    plain, _, _ = programs
    r = subprocess.run([plain] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _judge(r.stdout)


def test_key_set_plan_and_lookup_under_asan_and_ubsan(programs, files):
    _, san, err = programs
    assert san is not None, "the host sanitizer build of the check program failed:\n" + err[-4000:]
    r = subprocess.run([san] + files, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    _judge(r.stdout)

