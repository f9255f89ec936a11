"""AddressSanitizer + UndefinedBehaviorSanitizer over the .wtns container check that plk_wtns_decode and plk_prove_wtns make on the host
before anything reaches the device (wtns_container, circuit.cpp): a stand-alone program (tests/host/sanitize_wtns.cpp, its own main, gcc,
no HIP, no GPU) feeds it the golden witness, every truncation of its head, every overwrite of a container byte and random mutations, and
holds it against plk_circuit_load's parser on the same bytes."""
import os
import shutil
import subprocess

import pytest

import plonkit_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_wtns_container_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_wtns")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                           os.path.join(ROOT, "tests", "host", "sanitize_wtns.cpp"), "-o", exe])
    c = pa.Circuit.from_files(os.path.join(GOLD, "circuit.r1cs.json"), os.path.join(GOLD, "witness.json"))
    wt = tmp_path / "witness.wtns"
    wt.write_bytes(c.export("wtns"))
    r = subprocess.run([exe, str(wt), "4000"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "0 disagreements" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout + r.stderr)[-4000:]
