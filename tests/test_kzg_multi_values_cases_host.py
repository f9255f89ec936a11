"""-m "not gpu": the Python-integer model of the multi-point openings from values (tests/gen/kzg_multi_values_cases.py: one inversion for
all points, barycentric sums, the quotient in values with its positions on the domain) against THE DEFINITION of
tests/gen/kzg_multi_cases.py — interpolate r_i, long-divide by Z_{S_i} — through an integer NTT.  Pure Python, exact.  Four plausible
wrong arrangements are shown to fail on at least one case each."""
import random

import pytest

from tests.gen import kzg_multi_cases as km
from tests.gen import kzg_multi_values_cases as kv

R = km.R


def _cases(log_n):
    """(name, coefficient lists, points, sets, gamma, u): the mask families at shapes that fit, over drawn and directed points"""
    n = 1 << log_n
    rng = random.Random(77 + log_n)
    out = []
    shapes = ((1, 1), (3, 2), (4, 3), (8, 4)) if log_n >= 3 else ((1, 1), (3, 2))
    for m, p in shapes:
        polys = [km.poly(km.POLY_KINDS[i % 4] if i < 3 else "random", n, 100 * log_n + i) for i in range(m)]
        if m > 1:
            polys[-1] = list(polys[0])                                # the same polynomial twice
        for name, sets in sorted(km.mask_families(m, p, seed=m + p).items()):
            points = km.point_cases(log_n, p, seed=m + len(out))      # 1, r - 1, omega^3, omega^(N-1), 0, 42 among them
            points = [t for k, t in enumerate(points) if t not in points[:k]]
            if len(points) < p:
                continue
            dom = kv.domain(log_n)
            for u in (rng.randrange(R), 0, 1, dom[5 % n], points[0]):
                out.append(("%s %dx%d u=%x" % (name, m, p, u % 997), polys, points, sets, rng.randrange(R), u))
    for points in kv.directed_points(log_n):
        points = [t for k, t in enumerate(points) if t not in points[:k]][:min(8, n)]
        p, m = len(points), max(len(points), 2)
        polys = [km.poly("random", n, 900 + 10 * log_n + i) for i in range(m)]
        out.append(("directed %d" % p, polys, points, km.random_masks(m, p, 3), rng.randrange(R), points[-1]))
        out.append(("directed all %d" % p, polys, points, km.all_masks(m, p), R - 1, rng.randrange(R)))
    return out


def _pad(c, n):
    return (list(c) + [0] * n)[:n]


@pytest.mark.parametrize("log_n", kv.MODEL_LOG_SIZES)
def test_the_ntt_of_the_model_is_an_evaluation(log_n):
    n = 1 << log_n
    f = km.poly("random", n, log_n)
    vals = kv.ntt(f, log_n)
    assert vals == [km.horner(f, x) for x in kv.domain(log_n)]
    assert kv.ntt(vals, log_n, inverse=True) == f
    assert sum(x * kv.inv((x - kv.domain(log_n)[1]) % R) for k, x in enumerate(kv.domain(log_n)) if k != 1) % R == kv.rest_sum(log_n)


@pytest.mark.parametrize("log_n", kv.MODEL_LOG_SIZES)
def test_values_model_against_the_definition(log_n):
    n = 1 << log_n
    seen_on, seen_u_on = 0, 0
    for name, polys, points, sets, gamma, u in _cases(log_n):
        vals = [kv.ntt(f, log_n) for f in polys]
        o = kv.opening(vals, log_n, points, sets, gamma, u)
        assert o["evals"] == km.evaluations(polys, points, sets), name
        h = km.h_by_definition(polys, points, sets, gamma)
        assert kv.ntt(o["h"], log_n, inverse=True) == _pad(h, n), name
        assert kv.ntt(o["q2"], log_n, inverse=True) == _pad(km.second_quotient_by_definition(polys, h, points, sets, gamma, u), n), name
        seen_on += sum(k is not None for k in o["ks"])
        if kv.on_domain(u, log_n):                                    # the identity the library holds against the arrays at position k
            seen_u_on += 1
            k = kv.domain(log_n).index(u)
            c, z_t = km.c_values(points, sets, gamma, u)
            assert (sum(ci * f[k] for ci, f in zip(c, vals)) - z_t * o["h"][k]) % R == o["v"], name
    assert seen_on and seen_u_on


def test_the_operator_alone_with_points_on_the_domain():
    log_n, n = 4, 16
    rng = random.Random(5)
    polys = [km.poly("random", n, 40 + i) for i in range(5)]
    vals = [kv.ntt(f, log_n) for f in polys]
    for points in kv.directed_points(log_n) + [[3, 3], [1, 1, 7]]:    # equal points are legal for the operator on its own
        coef = [[rng.randrange(R) if rng.randrange(4) else 0 for _ in points] for _ in polys]
        coef[1] = [0] * len(points)
        got = kv.quotient_values(vals, log_n, points, coef)
        assert kv.ntt(got, log_n, inverse=True) == km.quotient_multi(polys, points, coef), points


@pytest.mark.parametrize("wrong", kv.WRONG)
def test_wrong_arrangements_fail(wrong):
    failed = 0
    for log_n in (1, 3):
        n = 1 << log_n
        for name, polys, points, sets, gamma, u in _cases(log_n):
            vals = [kv.ntt(f, log_n) for f in polys]
            good, bad = kv.opening(vals, log_n, points, sets, gamma, u), kv.opening(vals, log_n, points, sets, gamma, u, wrong)
            failed += (good["evals"], good["h"], good["q2"]) != (bad["evals"], bad["h"], bad["q2"])
    assert failed, wrong
