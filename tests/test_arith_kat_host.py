"""Known answers for the header-level primitives, HOST run: tests/host/arith_kat.hip applies each primitive of field_dev.h, field29_dev.h, ec_dev.h,
ec29_dev.h, glv_dev.h, g1_mul_dev.h (xyzzw_add_mixed_os) and msm_shape.h (recode17, extract_bits) to the cases of tests/gen/arith_cases.py on the CPU, and every result is compared
with that module's integer model: the exact Montgomery value where the header defines one, canonical residues, the affine BN254 group law, the
stated digit ranges; plus the output invariants of ec29_dev.h (limbs normalised, x, y < 6p, zz, zzz < 1.3p) after single operations and after every
step of 32-step chains.  All comparisons are exact.  The operands are directed (limb boundaries of both layers, operands at the top of each
documented lazy contract, ties of the conditional subtractions, multiples of p for the zero tests, forged operands for the false-positive branch of
the mixed addition) plus 4096 random cases per primitive.  No GPU involved (hipcc only compiles): the host build of these functions is what lets the
cases and the model be debugged anywhere; tests/test_gpu_arith_kat.py runs the same cases through the device build and compares limb for limb.

NOT covered here, because the functions are __device__ only (the GPU test covers them): xyzzw_export, store_xyzzw / load_xyzzw,
ec29_quad_dev.h's xyzzw_add_dist, quad_distribute and quad_gather, and g1_mul_dev.h's g1_mul_scalar, g1_mul_scalar_iso and g1_mul_scalar_iso8
(their window tables live in LDS).  What this file does check of those three is their MODEL: the fixed-base multiplication that gives the expected
points agrees with the CPU oracle's double-and-add, and the scalars chosen for them have the splits and recodings they are chosen for."""
import random
import shutil

import numpy as np
import pytest

from oracle import oracle_lib as ol
from tests.gen import arith_cases as ac

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# every primitive the host run must hold cases for, per field it is instantiated with (0 = Fr / FrW, 1 = Fq / FqW)
BOTH_FIELDS = ["F_ADD", "F_SUB", "F_NEG", "F_DBL", "F_MUL", "F_SQR", "F_INV", "F_TO_CANONICAL", "F_FROM_CANONICAL", "F_FROM_U64", "F_POW_U64",
               "W_MULW", "W_MULW2", "W_SQRW", "W_SQRW2", "W_MUL2ADDW", "W_MULSUM3W", "W_MUL_TW3", "W_MUL_TW3_2", "W_MULW_OS", "W_SQRW_OS",
               "W_MUL2ADDW_OS", "W_SUB2", "W_SUB4", "W_SUB6", "W_NEG2", "W_NORMW", "W_CSUB_P", "W_REDUCE_FULL", "W_REDUCE_SMALL", "W_IS_ZERO_MOD_P",
               "W_MAYBE_ZERO_MOD_P", "W_UNPACK", "W_PACK", "W_W_FROM_S", "W_S_FROM_W"]
CURVE = ["E_XYZZ_ADD_MIXED", "E_XYZZ_ADD", "E_XYZZ_DOUBLE", "E_XYZZW_ADD_MIXED", "E_XYZZW_ADD", "E_XYZZW_DOUBLE", "E_XYZZW_DOUBLE_AFFINE",
         "E_XYZZW_ADD_MIXED_SPECIAL", "E_XYZZW_CHAIN", "E_XYZZW_ADD_MIXED_OS"]
SCALAR = ["G_GLV_SPLIT", "G_GLV_DIGITS", "G_GLV_DIGITS4", "G_RECODE17", "G_EXTRACT_BITS"]
DEVICE_ONLY = ["E_XYZZW_EXPORT", "E_XYZZW_STORE_LOAD", "G_MUL_SCALAR", "G_MUL_SCALAR_ISO", "G_MUL_SCALAR_ISO8", "Q_ADD_DIST", "Q_DISTRIBUTE_GATHER0",
               "Q_DISTRIBUTE_GATHER1", "Q_DISTRIBUTE_GATHER2", "Q_DISTRIBUTE_GATHER3"]
COVERAGE = sorted([(n, f) for n in BOTH_FIELDS for f in (0, 1)] + [(n, 1) for n in CURVE] + [(n, 0) for n in SCALAR])


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("arith_kat_host"))
    exe = ac.build_program(work)
    groups = ac.generate(device=False)
    outs, summary = ac.run_program(exe, groups, work, host=True)
    return groups, outs, summary


def test_every_primitive_has_cases(host_run):
    groups, outs, summary = host_run
    have = sorted((g.name, g.field) for g in groups)
    assert have == COVERAGE == ac.expected_coverage(device=False)
    assert sorted(n for n, v in ac.OPS.items() if v[4]) == DEVICE_ONLY
    for g in groups:                                                         # (a chain case is 32 dependent operations)
        assert len(g.cases) * (ac.CHAIN_STEPS if g.name == "E_XYZZW_CHAIN" else 1) >= ac.RANDOM_CASES, (g.name, len(g.cases))
    assert "%d groups, %d cases on the host" % (len(groups), sum(len(g.cases) for g in groups)) in summary, summary


@pytest.mark.parametrize("name,field", COVERAGE, ids=["%s-%s" % (n, ac.FIELD_NAME[f]) for n, f in COVERAGE])
def test_host_results_equal_the_integer_model(host_run, name, field):
    groups, outs, _ = host_run
    (g, o), = [(g, o) for g, o in zip(groups, outs) if (g.name, g.field) == (name, field)]
    assert len(o) == len(g.cases)                                            # generated == run ...
    assert ac.check_group(g, o) == len(g.cases)                              # ... == checked: nothing is filtered after generation


def test_scalar_multiplication_model_matches_the_oracle():
    """g_mul, the expected value of the G_MUL_SCALAR* cases, against the oracle library's double-and-add on the same scalars"""
    rng = random.Random(85)
    G = ol.g1_generator()
    for k in [0, 1, 2, 255, 256, ac.R_MOD - 1, ac.LAMBDA, 1 << 128] + [rng.randrange(ac.R_MOD) for _ in range(40)]:
        want = ac.g_mul(k)
        assert np.array_equal(ol.g1_mul(G, k), ol.g1_from_ints(*(want or (0, 0)))), hex(k)


def test_directed_scalars_of_the_multiplications():
    """the list asked of the G1 multiplications is what it says: every named scalar is there, the chosen splits and recodings hold in integers,
    and every domain size contributes its 1 / n, its twiddles and their products"""
    sc = ac.mul_scalars(random.Random(1))
    ks = [k for k, _ in sc]
    r, lam = ac.R_MOD, ac.LAMBDA
    for k in list(range(18)) + [r - 1, r - 2, (r - 1) // 2, lam, lam + 1, lam - 1, r - lam, 1 << 127, (1 << 128) + 1, (1 << 128) - 1]:
        assert k in ks, hex(k)
    assert sum(1 for k, why in sc if why == "k2 == 0" and ac.glv_split_model(k)[1] == 0 and ac.glv_split_model(k)[0] == k) >= 5
    assert sum(1 for k, why in sc if why == "k2 < 0" and ac.glv_split_model(k)[3]) >= 12

    def digits(v, bits):                                     # the signed recoding glv_dev.h describes, in integers
        out, carry = [], 0
        while v or carry:
            d = (v & ((1 << bits) - 1)) + carry
            v >>= bits
            carry = 1 if d > 1 << (bits - 1) else 0
            out.append(d - (carry << bits))
        return out
    for bits, least in ((4, 30), (3, 41)):
        ext = [k for k, why in sc if why == "extreme digits, %d-bit windows" % bits]
        seen = set()
        for k in ext:
            k1, k2, n1, n2 = ac.glv_split_model(k)
            assert not n1 and not n2
            for half in (k1, k2):
                d = digits(half, bits)
                hi, lo = 1 << (bits - 1), 1 - (1 << (bits - 1))
                kind = hi if d[0] == hi else lo
                assert len(d) >= least and all(v == kind for v in d[:least]), (bits, d)
                seen.add(kind)
        assert len(ext) == 4 and seen == {1 << (bits - 1), 1 - (1 << (bits - 1))}
    for log_n in range(1, ac.MAX_LOG_N + 1):
        n_inv, w_inv = pow(1 << log_n, -1, r), pow(ac.omega(log_n), -1, r)
        assert pow(ac.omega(log_n), 1 << log_n, r) == 1 and pow(ac.omega(log_n), 1 << (log_n - 1), r) == r - 1
        assert n_inv in ks and w_inv in ks and w_inv * n_inv % r in ks
        assert sum(1 for _, why in sc if why.startswith("omega^-") and why.endswith("log_n %d" % log_n)) >= (2 if log_n > 1 else 0)
