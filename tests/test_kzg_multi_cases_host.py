"""-m "not gpu": the Python-integer model of the multi-point openings (tests/gen/kzg_multi_cases.py) against itself.  The first quotient by
the definition (interpolation, long division by Z_{S_i}) equals the grouped formula the kernel implements; the second quotient by long
division equals the same operator at one point; with tau = 42 the verifier's equation holds in the exponent; and the case list tells the
right arrangement from three wrong ones (gamma indexed by point, weights left out, Z_{S_i}(u) in place of Z_{T \\ S_i}(u))."""
import random

import pytest

from tests.gen import kzg_multi_cases as km

R = km.R
GAMMA = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80919 % R


def _polys(m, n, seed):
    return [km.poly(km.POLY_KINDS[i % 4] if i % 5 == 2 else "random", n, seed + i) for i in range(m)]


def _shapes():
    for n in km.MODEL_SIZES:
        for m, p in ((1, 1), (3, 2), (4, 3), (8, 4), (9, 8)):
            yield n, m, p


@pytest.mark.parametrize("n,m,p", list(_shapes()))
def test_the_definition_equals_the_grouped_formula(n, m, p):
    log_n = max(n - 1, 1).bit_length()
    points = km.point_cases(log_n, p)                               # 0, 1, r - 1, 42 and domain points among them
    polys = _polys(m, n, 100 * n + m)
    for name, sets in km.mask_families(m, p).items():
        assert km.check_sets(points, sets) is None, name
        h = km.h_by_definition(polys, points, sets, GAMMA)
        assert h == km.h_grouped(polys, points, sets, GAMMA), (name, n, m, p)
        assert h[n - 1] == 0
        for u in (0, points[0], 12345678901234567890, R - 1):
            q2 = km.second_quotient_by_definition(polys, h, points, sets, GAMMA, u)
            assert q2 == km.second_quotient(polys, h, points, sets, GAMMA, u), (name, n, m, p, u)


@pytest.mark.parametrize("m,p", km.HOST_SHAPES + ((4, 3),))
def test_the_verifier_equation_holds_in_the_exponent(m, p):
    n = 24
    points = km.point_cases(5, p)
    polys = _polys(m, n, 7 * m + p)
    cms = [km.horner(f, km.TAU) for f in polys]
    rng = random.Random(m * 10 + p)
    for name, sets in km.mask_families(m, p).items():
        for u in (0, points[p - 1], km.TAU, rng.randrange(R)):
            o = km.opening(polys, points, sets, GAMMA, u)
            assert km.verifier_exponent(cms, points, sets, o["evals"], GAMMA, u, o["w"], o["w2"]) == 0, (name, u)
            # one evaluation changed: the equation fails
            i = m - 1
            j = km.members(sets[i], p)[0]
            bad = [row[:] for row in o["evals"]]
            bad[i][j] = (bad[i][j] + 1) % R
            # (u equal to ANOTHER point makes r_i(u) that point's evaluation alone, or c_i zero: soundness rests on u being drawn after W)
            if all(u != points[l] for l in range(p) if l != j):
                assert km.verifier_exponent(cms, points, sets, bad, GAMMA, u, o["w"], o["w2"]) != 0, (name, u)


def test_each_wrong_arrangement_is_told_apart_by_some_case():
    """every wrong variant fails the verifier's equation on at least one family of every multi-point shape, and on the PLONK-like masks"""
    for m, p in ((3, 2), (8, 4), (32, 8)):
        points, polys = km.point_cases(5, p), _polys(m, 24, m)
        cms = [km.horner(f, km.TAU) for f in polys]
        for wrong in km.WRONG:
            told = 0
            for sets in km.mask_families(m, p).values():
                o = km.opening(polys, points, sets, GAMMA, 99, wrong=wrong)
                told += km.verifier_exponent(cms, points, sets, o["evals"], GAMMA, 99, o["w"], o["w2"]) != 0
            assert told, (m, p, wrong)


def test_the_refused_sets():
    pts = [5, 6, 7]
    assert km.check_sets(pts, [1, 2, 4]) is None
    assert km.check_sets([5, 6, 5], [1, 2, 4]) == "duplicate point"
    assert km.check_sets(pts, [1, 0, 6]) == "empty set"
    assert km.check_sets(pts, [1, 2, 12]) == "bit above"
    assert km.check_sets(pts, [1, 2, 3]) == "unused point"


def test_the_mask_families_are_what_their_names_say():
    assert km.plonk_like_masks(8) == [5, 1, 1, 1, 1, 1, 3, 3]
    assert km.singleton_masks(3, 3) == [1, 2, 4]
    for seed in range(4):
        assert km.check_sets(list(range(8)), km.random_masks(32, 8, seed)) is None
