"""-m "not gpu": the Python-integer model of the one-pass openings (tests/gen/fk20_cases.py) against the definition of an opening, and a
proof on the CPU that the cases discriminate.

1. For N = 1 .. 32 the model's DFT_N(h), with h taken through the two arrangements and the 2N correlation, equals
   (f(tau) - f(omega^i)) / (tau - omega^i) for random f and for the directed ones (zero, constant, only f_{N-1}, only f_1); h through the
   correlation equals h by its definition, h_{N-1} = 0 included.
2. For every deliberately wrong arrangement (t_{2N-j} swapped for t_j, the 1 / 2N dropped, the upper half taken) some case differs."""
import pytest

from tests.gen import fk20_cases as fk
from tests.gen import kzg_cases as kc

R = kc.R
CASES = [(log_n, kind, tau) for log_n in fk.MODEL_LOG_NS for kind in fk.POLY_KINDS for tau in fk.TAUS]


def test_the_quadratic_transform_is_the_models_fft():
    for log_n in (1, 3, 6):
        v = fk.poly("random", log_n, seed=9)
        assert fk.dft(v, kc.omega(log_n)) == kc.evaluate_on_domain(v, log_n)
        assert fk.idft(fk.dft(v, kc.omega(log_n)), kc.omega(log_n)) == v


@pytest.mark.parametrize("log_n", fk.MODEL_LOG_NS)
def test_the_correlation_gives_h_and_the_openings(log_n):
    n = 1 << log_n
    for kind in fk.POLY_KINDS:
        for tau in fk.TAUS:
            what = (log_n, kind, tau)
            assert pow(tau, n, R) != 1, what                                         # tau off the domain: the definition divides by tau - omega^i
            f = fk.poly(kind, log_n)
            h = fk.quotient_commitments(f, tau)
            assert len(h) == n and h[n - 1] == 0, what
            assert fk.correlation_h(f, tau, log_n) == h, what
            want = fk.openings_by_definition(f, tau, log_n)
            assert fk.openings(f, tau, log_n) == want, what
            # the same proofs as one synthetic division per point (what plk_kzg_open_dev commits to)
            for i in (0, n // 2, n - 1):
                q = kc.divide_by_linear(f, pow(kc.omega(log_n), i, R))
                assert kc.horner(q, tau) == want[i], what
            if kind in ("zero", "constant"):
                assert want == [0] * n, what                                          # the point at infinity everywhere
            if kind == "top_only" and n > 1:
                assert all(want), what


def test_the_arrangements_are_what_the_issue_states():
    for log_n in fk.MODEL_LOG_NS:
        n = 1 << log_n
        c, t = fk.c_sources(log_n), fk.t_sources(log_n)
        assert len(c) == len(t) == 2 * n
        assert [s for s in c if s is not None] == list(range(1, n))                  # f_1 .. f_{N-1}, f_0 nowhere
        assert sorted(s for s in t if s is not None) == list(range(max(n - 1, 0)))   # s_0 .. s_{N-2}: N - 1 key points
        assert all(s is None for s in c[max(n - 1, 0):]) and all(s is None for s in t[1:n + 2])


@pytest.mark.parametrize("wrong", fk.WRONG_VARIANTS)
def test_the_cases_catch_the_wrong_variant(wrong):
    caught = [c for c in CASES if fk.openings(fk.poly(c[1], c[0]), c[2], c[0], wrong=wrong) != fk.openings(fk.poly(c[1], c[0]), c[2], c[0])]
    assert caught, wrong
    assert {c[1] for c in caught} <= {"top_only", "f1_only", "random"}, caught       # zero and constant have h = 0 whatever the arrangement
    assert any(c[1] == "random" for c in caught), caught
