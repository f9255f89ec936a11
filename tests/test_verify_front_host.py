"""The device front end of the verifier (plonkit_amd/csrc/verify_front_dev.h: Keccak-f[1600], the rolling transcript, the proof parser and
the flattening that vm_front_kernel runs, one proof per lane) compiled for the HOST — its functions are __host__ __device__ — against the
host code it restates (tests/host/verify_front_check.hip: keccak256 on every length 0..135, RollingKeccak over random sequences,
verify_terms_parsed on the golden proof, cuts at every field boundary, count fields, q and r, flag bits, wrong keys, 3000 byte mutations).
The tampered proofs and keys of tests/test_verify_terms_host.py are made here with the oracle and handed over as files.  The same program
is built a second time with host AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone executable (its own main, nothing loaded
into Python): every proof sits in a heap block of exactly its own length, so a read past the end is reported.  No GPU involved."""
import os
import re
import shutil
import subprocess

import pytest

from oracle import plonk_oracle as po

R_MOD = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "verify_front_check.hip")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def _with(proof, **changes):
    P = po.read_proof(proof)
    for k, v in changes.items():
        setattr(P, k, v(getattr(P, k)))
    return po.write_proof(P)


def tampering_cases(proof):
    """the tampering cases of tests/test_verify_terms_host.py: name -> tampered proof bytes"""
    bump = lambda x: (x + 1) % R_MOD
    bump_first = lambda xs: [bump(xs[0])] + list(xs[1:])
    swap01 = lambda xs: [xs[1], xs[0]] + list(xs[2:])
    P0 = po.read_proof(proof)
    cases = {"inputs": bump_first, "wire_values_at_z": bump_first, "wire_values_at_z_omega": bump_first,
             "permutation_polynomials_at_z": bump_first, "grand_product_at_z_omega": bump,
             "quotient_polynomial_at_z": bump, "linearization_polynomial_at_z": bump,
             "wire_commitments": swap01, "quotient_poly_commitments": swap01,
             "grand_product_commitment": lambda c: P0.wire_commitments[0],
             "opening_at_z_proof": lambda c: P0.opening_at_z_omega_proof,
             "opening_at_z_omega_proof": lambda c: P0.opening_at_z_proof}
    return {f: _with(proof, **{f: c}) for f, c in cases.items()}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the check program twice, compiled side by side: plain, and host code only with the host sanitizers (no device code, GPU sanitizing off)"""
    d = tmp_path_factory.mktemp("verify_front")
    plain, san = str(d / "verify_front_check"), str(d / "verify_front_check_san")
    jobs = [subprocess.Popen(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", SRC, "-o", plain], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(["hipcc", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17",
                              SRC, "-o", san], stderr=subprocess.PIPE, text=True)]
    errs = [j.communicate()[1] for j in jobs]
    assert jobs[0].returncode == 0, errs[0][-4000:]
    return plain, (san if jobs[1].returncode == 0 else None), errs[1]


@pytest.fixture(scope="module")
def listed(tmp_path_factory, golden_dir):
    """vk.bin, proof.bin and the list file of the cases made with the oracle: (vk, proof, list, count)"""
    d = tmp_path_factory.mktemp("verify_front_cases")
    vkp, pp = os.path.join(golden_dir, "vk.bin"), os.path.join(golden_dir, "proof.bin")
    vk, proof = open(vkp, "rb").read(), open(pp, "rb").read()
    lines = []
    for name, bad in tampering_cases(proof).items():
        assert bad != proof, name
        f = d / (name + ".proof.bin")
        f.write_bytes(bad)
        lines += ["%s %s 0" % (vkp, f), "%s %s 1" % (vkp, f)]
    V = po.read_vk(vk)
    V.permutation_commitments = [V.permutation_commitments[1], V.permutation_commitments[0]] + list(V.permutation_commitments[2:])
    for k, other in enumerate((po.write_vk(V), vk[:-256] + vk[-128:] + vk[-256:-128])):      # wrong keys of the same shape
        f = d / ("other%d.vk.bin" % k)
        f.write_bytes(other)
        lines.append("%s %s 0" % (f, pp))
    P = po.read_proof(proof)
    P.inputs = list(P.inputs) + [5]
    f = d / "more_inputs.proof.bin"
    f.write_bytes(po.write_proof(P))
    lines.append("%s %s 0" % (vkp, f))
    lst = d / "cases.txt"
    lst.write_text("\n".join(lines) + "\n")
    return vkp, pp, str(lst), len(lines)


def _judge(out, count):
    assert "0 mismatches" in out, out[-4000:]
    assert "%d listed cases" % count in out, out[-2000:]
    m = re.search(r"fuzz: (\d+) cases, host states: (\d+) invalid, (\d+) go on, (\d+) malformed", out)
    assert m, out[-2000:]
    cases, split = int(m.group(1)), [int(m.group(k)) for k in (2, 3, 4)]
    assert cases >= 3000 and sum(split) == cases
    assert all(10 * s >= cases for s in split), split            # on the HOST's answers: the run cannot pass on malformed proofs alone


def test_device_front_end_on_the_host(programs, listed):
    plain, _, _ = programs
    vk, proof, lst, count = listed
    r = subprocess.run([plain, vk, proof, lst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _judge(r.stdout, count)


def test_device_front_end_under_asan_and_ubsan(programs, listed):
    _, san, err = programs
    assert san is not None, "the host sanitizer build of the check program failed:\n" + err[-4000:]
    vk, proof, lst, count = listed
    r = subprocess.run([san, vk, proof, lst], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    _judge(r.stdout, count)
