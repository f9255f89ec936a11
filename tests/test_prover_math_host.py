"""-m "not gpu": the host scalar algebra of prover rounds 4 and 5 (plonkit_amd/csrc/prover_math.h: the shared inversion for 1/z, 1/(z omega) and
L_0(z), the refusals of z, f_z and f_sigma, the nine linearisation coefficients, the twelve-plus-two opening coefficients, the constants of the coset
iNTT's combine step) — tests/host/prover_math_check.cpp is built as a stand-alone program with AddressSanitizer and UBSan and run directly (it is not
loaded into Python).  The inputs are the challenges and evaluations of the reference's golden proof (tests/golden/proof.bin, the one
tests/test_oracle_golden.py pins the oracle to); the expected values are oracle/plonk_oracle.py's for that proof."""
import os
import shutil
import subprocess

import pytest

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "prover_math_check.cpp")
HEADER = os.path.join(ROOT, "plonkit_amd", "csrc", "prover_math.h")


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prover_math") / "prover_math_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _hex(v):
    return "%064x" % (v % R_MOD)


def _run(program, lines):
    r = subprocess.run([program], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout.split("\n")[:-1]


def _ints(line):
    return [int(x, 16) for x in line.split()]


@pytest.fixture(scope="module")
def golden(golden_dir, golden_crs):
    r1cs = po.load_r1cs_json(os.path.join(golden_dir, "circuit.r1cs.json"))
    w = po.load_witness_json(os.path.join(golden_dir, "witness.json"))
    P, dbg = po.prove(r1cs, w, golden_crs, return_debug=True)
    assert po.write_proof(P) == open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    return P, dbg


def test_the_header_is_host_only():
    text = open(HEADER, encoding="utf-8").read()
    assert "hip/" not in text and "getenv" not in text
    assert [line.split()[1] for line in text.splitlines() if line.startswith("#include")] == ["<stdint.h>", '"hostmath.h"']


def test_rounds_4_and_5_of_the_golden_proof(program, golden):
    P, dbg = golden
    N = P.n + 1
    om = ol.omega(N.bit_length() - 1)
    z, v, alpha, beta, gamma = (dbg[k] for k in ("z", "v", "alpha", "beta", "gamma"))
    wz, sz = P.wire_values_at_z, P.permutation_polynomials_at_z
    ev = wz + P.wire_values_at_z_omega + sz + [P.quotient_polynomial_at_z, P.grand_product_at_z_omega]
    out = _run(program, ["round %d %s" % (N, " ".join(_hex(x) for x in [om, alpha, beta, gamma, z, v] + ev)),
                         "point %d %s %s" % (N, _hex(om), _hex(z))])
    assert len(out) == 5
    zN = pow(z, N, R_MOD)
    assert _ints(out[0]) == [dbg["l0_z"], dbg["fz"], dbg["fs"]]
    # r(x) = q_const + a q_a + b q_b + c q_c + d q_d + a b q_m + d(z omega) q_dnext + f_z z(x) - f_sigma sigma_3(x)   (prove_columns, round 4)
    assert _ints(out[1]) == [1, wz[0], wz[1], wz[2], wz[3], wz[0] * wz[1] % R_MOD, P.wire_values_at_z_omega[0], dbg["fz"], (R_MOD - dbg["fs"]) % R_MOD]
    # t_0..t_3 by powers of z^N, then r, the four wires and three sigmas by v .. v^8; z(x) and d(x) at z omega by v^9, v^10   (round 5)
    assert _ints(out[2]) == [pow(zN, k, R_MOD) for k in range(4)] + [pow(v, k, R_MOD) for k in range(1, 9)]
    assert _ints(out[3]) == [pow(v, 9, R_MOD), pow(v, 10, R_MOD)]
    head, *point = out[4].split(" ", 1)
    assert head == "ok"
    assert _ints(point[0]) == [pow(z, -1, R_MOD), pow(z * om % R_MOD, -1, R_MOD), zN, dbg["l0_z"]]


def test_a_challenge_in_the_domain_or_zero_is_refused(program, golden):
    P, _ = golden
    N = P.n + 1
    om = ol.omega(N.bit_length() - 1)
    out = _run(program, ["point %d %s %s" % (N, _hex(om), _hex(z)) for z in (0, 1, om, pow(om, N - 1, R_MOD), 2)])
    assert out[:4] == ["refused challenge z = 0", "refused challenge z = 1", "refused challenge z^N = 1", "refused challenge z^N = 1"]
    assert out[4].startswith("ok ")


@pytest.mark.parametrize("log_n", [1, 3, 12, 20])
def test_icoset_constants(program, log_n):
    """i^-1 (i = omega_4) and 7^(-N c) / 4, c = 0 .. 3: one derivation for a setup's cache and for plk_icoset4_coset_major_dev"""
    N = 1 << log_n
    out = _run(program, ["icoset %d %s" % (log_n, _hex(ol.omega(2)))])
    g = pow(pow(po.COSET_GEN, N, R_MOD), -1, R_MOD)
    assert _ints(out[0]) == [pow(ol.omega(2), -1, R_MOD)] + [pow(4, -1, R_MOD) * pow(g, c, R_MOD) % R_MOD for c in range(4)]
