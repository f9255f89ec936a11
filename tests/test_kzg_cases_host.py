"""-m "not gpu": the Python-integer model of the KZG opening helpers (tests/gen/kzg_cases.py) against the oracle, and a proof on the CPU
that the case tables discriminate.

1. The model against the oracle (ol.omega, ol.ntt, ol.poly_eval, ol.poly_div_linear) for every case: interpolation, evaluation from
   values, the quotient in values — and in particular the in-domain position q(omega^k), which is compared with
   interpolate -> divide -> evaluate on the domain, so that nobody has to take the identity on trust.
2. For every deliberately wrong variant of the quotient (no in-domain substitution, f_k from the formula, the omega^i factor dropped,
   k off by one) some case of the tables differs from the right answer."""
import numpy as np
import pytest

from oracle import oracle_lib as ol
from tests.gen import kzg_cases as kc

R = kc.R


def _cases():
    for log_n in kc.MODEL_LOG_NS:
        for zname, z in kc.z_cases(log_n).items():
            for kind in kc.POLY_KINDS:
                yield log_n, zname, z, kind


CASES = list(_cases())


@pytest.mark.parametrize("log_n", sorted(set(kc.HELPER_LOG_NS) | {kc.LARGE_LOG_N, 28}))
def test_omega_is_the_oracles(log_n):
    assert kc.omega(log_n) == ol.omega(log_n)


def test_every_model_quantity_against_the_oracle():
    assert kc.R == ol.R_MOD
    for log_n, zname, z, kind in CASES:
        what = (log_n, zname, kind)
        vals = kc.poly_values(kind, log_n, z)
        coeffs = kc.interpolate(vals, log_n)
        assert coeffs == ol.fr_ints(ol.ntt(ol.fr_vec(vals), log_n, inverse=True)), what
        y = kc.evaluate_values(vals, log_n, z)
        assert y == ol.poly_eval(ol.fr_vec(coeffs), z), what
        assert y == kc.horner(coeffs, z), what
        q = kc.divide_by_linear(coeffs, z)
        assert q == ol.fr_ints(ol.poly_div_linear(ol.fr_vec(coeffs), z)), what
        # the quotient in values, the in-domain position included, is the quotient polynomial on the domain
        assert kc.quotient_values(vals, log_n, z) == ol.fr_ints(ol.ntt(ol.fr_vec(q), log_n)), what
        assert kc.quotient_values(vals, log_n, z, y=y) == kc.evaluate_on_domain(q, log_n), what


def test_x_minus_z_has_the_constant_quotient_one():
    for log_n in kc.MODEL_LOG_NS:
        for zname, z in kc.z_cases(log_n).items():
            assert kc.quotient_values(kc.poly_values("x_minus_z", log_n, z), log_n, z) == [1] * (1 << log_n), (log_n, zname)


@pytest.mark.parametrize("wrong", kc.WRONG_VARIANTS)
def test_the_cases_catch_the_wrong_variant(wrong):
    caught = [(log_n, zname, kind) for log_n, zname, z, kind in CASES
              if kc.quotient_values(kc.poly_values(kind, log_n, z), log_n, z, wrong=wrong) != kc.quotient_values(kc.poly_values(kind, log_n, z), log_n, z)]
    assert caught, wrong
    assert all(zname.startswith("omega^") or zname == "1" or (zname == "r-1") for _, zname, _ in caught), caught   # only in-domain points can tell


def test_case_tables_hold_what_the_gpu_tests_rely_on():
    z = kc.z_cases(12)
    assert {"random", "0", "1", "r-1", "42", "omega^0", "omega^1", "omega^2047", "omega^2048", "omega^N-1", "2N-th root"} <= set(z)
    assert "omega^2047" not in kc.z_cases(8) and "omega^N-1" in kc.z_cases(1)
    root = kc.z_cases(12)["2N-th root"]
    assert pow(root, 1 << 12, R) == R - 1 and pow(root, 1 << 13, R) == 1
    assert z["omega^0"] == 1 and kc.domain_index(12, z["omega^N-1"]) == 4095
    assert np.array_equal(ol.fr_vec([R - 1]), ol.fr_vec(kc.poly_values("all_r_minus_1", 1, 0)[:1]))
