"""-m "not gpu": plk_kzg_verify_multi (kzg_multi.hip; pure CPU) on the reference's own tests/golden/setup_2pow10.key (tau = 42) and its
G2 section.  The openings are built by the oracle alone: ol.msm over the golden key of the polynomials and of the two quotients that the
Python-integer model (tests/gen/kzg_multi_cases.py) forms — no product code makes what the product code checks.  One more test builds
tests/host/kzg_multi_plan_check.cpp, a stand-alone program over kzg_multi_plan.h with AddressSanitizer and UBSan, runs it directly (it is
not loaded into Python) and holds the weights, Z values and r_i(u) it prints against the model's numbers."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle.oracle_lib import Q_MOD, R_MOD
from tests.gen import kzg_multi_cases as km

ERR_ARG = 1
DEG = 24                                                         # coefficients per polynomial
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pa():
    import plonkit_amd
    return plonkit_amd


@pytest.fixture(scope="module")
def g2(golden_dir):
    return open(os.path.join(golden_dir, "setup_2pow10.key"), "rb").read()[-256:]


def _commit(crs, coeffs):
    return ol.msm(crs.g1[:len(coeffs)], ol.fr_vec(coeffs))


def _pts(points):
    return np.stack([ol.fr_mont(t) for t in points])


def _evals(rows):
    return np.stack([np.stack([ol.fr_mont(y) for y in row]) for row in rows])


def _opening(crs, polys, points, sets, gamma, u):
    """(commitments [m, 8], evals [m, p, 4], proof [2, 8]) from the model and the oracle's MSM"""
    o = km.opening(polys, points, sets, gamma, u)
    cms = np.stack([_commit(crs, f) for f in polys])
    return cms, _evals(o["evals"]), np.stack([_commit(crs, o["h"]), _commit(crs, o["q2"])])


def _verify(pa, g2, cms, points, sets, evals, gamma, u, proof):
    return pa.kzg_verify_multi(cms, _pts(points), sets, evals, ol.fr_mont(gamma), ol.fr_mont(u), proof, g2)


@pytest.fixture(scope="module")
def openings(golden_crs):
    rng = random.Random(20261021)
    out = {}
    for m, p in km.HOST_SHAPES:
        polys = [[rng.randrange(R_MOD) for _ in range(DEG)] for _ in range(m)]
        points = [rng.randrange(R_MOD) for _ in range(p)]
        sets = km.random_masks(m, p, 100 * m + p) if m > 1 else [1]
        gamma, u = rng.randrange(R_MOD), rng.randrange(R_MOD)
        out[(m, p)] = (points, sets, gamma, u) + _opening(golden_crs, polys, points, sets, gamma, u)
    return out


@pytest.mark.parametrize("shape", km.HOST_SHAPES)
def test_valid_openings(pa, g2, openings, shape):
    points, sets, gamma, u, cms, evals, proof = openings[shape]
    assert _verify(pa, g2, cms, points, sets, evals, gamma, u, proof) is True


@pytest.mark.parametrize("shape", km.HOST_SHAPES)
def test_every_evaluation_and_commitment_counts(pa, g2, openings, shape):
    points, sets, gamma, u, cms, evals, proof = openings[shape]
    m, p = shape
    for i in range(m):
        bad = cms.copy()
        bad[i] = ol.g1_add(bad[i], ol.g1_generator())
        assert _verify(pa, g2, bad, points, sets, evals, gamma, u, proof) is False, i
        for j in range(p):
            e = evals.copy()
            e[i, j] = ol.fr_mont(ol.fr_ints(e[i, j:j + 1])[0] + 1)
            inside = bool((sets[i] >> j) & 1)
            # inside the set the evaluation counts; outside it may be anything, even no residue at all
            assert _verify(pa, g2, cms, points, sets, e, gamma, u, proof) is (not inside), (i, j)
            if not inside and i < 2:
                e[i, j] = ol.int_to_limbs((1 << 256) - 1)
                assert _verify(pa, g2, cms, points, sets, e, gamma, u, proof) is True, (i, j)


@pytest.mark.parametrize("shape,what", [(s, w) for s in km.HOST_SHAPES for w in ("W", "W'", "gamma", "u", "set bit") if s != (1, 1) or w in ("W", "W'")])
def test_single_tampering_is_invalid(pa, g2, openings, shape, what):
    """(one polynomial at one point: gamma^0 = 1 whatever gamma is, the one set has no bit to flip, and L = (x - u) h makes W' = W an
    opening under EVERY u — the equation loses u — so that shape has the two proof points only)"""
    points, sets, gamma, u, cms, evals, proof = openings[shape]
    sets, proof = list(sets), proof.copy()
    if what == "W":
        proof[0] = ol.g1_add(proof[0], ol.g1_generator())
    elif what == "W'":
        proof[1] = ol.g1_add(proof[1], ol.g1_generator())
    elif what == "gamma":
        gamma = (gamma + 1) % R_MOD
    elif what == "u":
        u = (u + 1) % R_MOD
    else:                                                         # a flip that leaves the sets well-formed
        for i in range(len(sets)):
            for j in range(len(points)):
                flipped = sets[:i] + [sets[i] ^ (1 << j)] + sets[i + 1:]
                if km.check_sets(points, flipped) is None:
                    break
            else:
                continue
            break
        sets = flipped
        evals = evals.copy()
        evals[i, j] = ol.fr_mont(5)
    assert _verify(pa, g2, cms, points, sets, evals, gamma, u, proof) is False


def test_zero_and_constant_polynomials(pa, g2, golden_crs):
    points, sets, gamma, u = [3, 4], [3, 2, 1], 77, 1234567
    # zero polynomials: every commitment, W and W' are infinity
    zero = [[0] * DEG] * 3
    cms, evals, proof = _opening(golden_crs, zero, points, sets, gamma, u)
    assert not cms.any() and not proof.any()
    assert _verify(pa, g2, cms, points, sets, evals, gamma, u, proof) is True
    evals[1, 1] = ol.fr_mont(1)
    assert _verify(pa, g2, cms, points, sets, evals, gamma, u, proof) is False
    # constants: W and W' are infinity, the commitments are not
    const = [[7] + [0] * (DEG - 1), [8] + [0] * (DEG - 1), [0] * DEG]
    cms, evals, proof = _opening(golden_crs, const, points, sets, gamma, u)
    assert cms[0].any() and not cms[2].any() and not proof.any()
    assert _verify(pa, g2, cms, points, sets, evals, gamma, u, proof) is True
    evals[0, 0] = ol.fr_mont(8)
    assert _verify(pa, g2, cms, points, sets, evals, gamma, u, proof) is False


def test_extreme_points_and_challenges(pa, g2, golden_crs):
    rng = random.Random(5)
    polys = [[rng.randrange(R_MOD) for _ in range(DEG)] for _ in range(3)] + [[R_MOD - 1] * DEG]
    points, sets = [0, R_MOD - 1, 12345], [7, 1, 2, 4]
    for gamma, u in ((1, 0), (R_MOD - 1, R_MOD - 1), (0, 12345), (99, 0), (99, 1)):      # u = 0, u in T (0, r - 1 and 12345), gamma = 0
        cms, evals, proof = _opening(golden_crs, polys, points, sets, gamma, u)
        assert _verify(pa, g2, cms, points, sets, evals, gamma, u, proof) is True, (gamma, u)


def _refused(pa, g2, *args):
    with pytest.raises(pa.PlkError) as e:
        _verify(pa, g2, *args)
    assert e.value.code == ERR_ARG, e.value
    return str(e.value)


def test_malformed_inputs_are_err_arg(pa, g2, openings):
    points, sets, gamma, u, cms, evals, proof = openings[(3, 2)]
    assert "equal" in _refused(pa, g2, cms, [points[0], points[0]], sets, evals, gamma, u, proof)
    assert "empty set" in _refused(pa, g2, cms, points, [sets[0], 0, sets[2]], evals, gamma, u, proof)
    assert "does not exist" in _refused(pa, g2, cms, points, [sets[0], sets[1], 4], evals, gamma, u, proof)
    assert "belongs to no set" in _refused(pa, g2, cms, points, [1, 1, 1], evals, gamma, u, proof)
    off = cms.copy(); off[1][4] ^= np.uint64(1)                   # y moved: off the curve
    assert "commitment 1" in _refused(pa, g2, off, points, sets, evals, gamma, u, proof)
    for k in range(2):
        badp = proof.copy(); badp[k][0] ^= np.uint64(1)
        assert "proof" in _refused(pa, g2, cms, points, sets, evals, gamma, u, badp)
    big = cms.copy(); big[0][:4] = ol.int_to_limbs(Q_MOD)         # x = q: not a coordinate
    _refused(pa, g2, big, points, sets, evals, gamma, u, proof)
    r_limbs, pts = ol.int_to_limbs(R_MOD), _pts(points)
    for args in ((np.stack([r_limbs, pts[1]]), sets, evals, ol.fr_mont(gamma), ol.fr_mont(u)),          # a point = r
                 (pts, sets, evals, r_limbs, ol.fr_mont(u)),                                           # gamma = r
                 (pts, sets, evals, ol.fr_mont(gamma), r_limbs)):                                      # u = r
        with pytest.raises(pa.PlkError) as e:
            pa.kzg_verify_multi(cms, args[0], args[1], args[2], args[3], args[4], proof, g2)
        assert e.value.code == ERR_ARG and "not below r" in str(e.value)
    i = 0
    j = km.members(sets[i], 2)[0]
    e = evals.copy(); e[i, j] = ol.int_to_limbs((1 << 256) - 1)   # an evaluation inside a set that is no residue
    assert "not below r" in _refused(pa, g2, cms, points, sets, e, gamma, u, proof)
    with pytest.raises(pa.PlkError) as err:                       # 33 commitments, 9 points
        pa.kzg_verify_multi(np.zeros((33, 8), dtype=np.uint64), pts[:1], [1] * 33, np.zeros((33, 1, 4), dtype=np.uint64), ol.fr_mont(1), ol.fr_mont(1), proof, g2)
    assert err.value.code == ERR_ARG
    with pytest.raises(pa.PlkError) as err:
        pa.kzg_verify_multi(cms[:1], _pts(range(9)), [511], np.zeros((1, 9, 4), dtype=np.uint64), ol.fr_mont(1), ol.fr_mont(1), proof, g2)
    assert err.value.code == ERR_ARG


def test_g2_refusals_are_plk_pairing_checks(pa, g2, openings):
    points, sets, gamma, u, cms, evals, proof = openings[(1, 1)]
    for at in (127, 255):
        bad = bytearray(g2); bad[at] ^= 1
        with pytest.raises(pa.PlkError) as mine:
            _verify(pa, bytes(bad), cms, points, sets, evals, gamma, u, proof)
        with pytest.raises(pa.PlkError) as theirs:
            pa.pairing_check(proof[0], bytes(bad[:128]), proof[0], bytes(bad[128:]))
        assert mine.value.code == theirs.value.code == ERR_ARG
        assert str(mine.value) == str(theirs.value) and "not on the twist" in str(mine.value)


# ------------------------------------------------------------------------------------------------ the header under the sanitizers
def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


@pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")
def test_the_plan_header_under_the_sanitizers_gives_the_models_numbers(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "kzg_multi_plan_check.cpp")
    exe = str(tmp_path / "kzg_multi_plan_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = random.Random(31)
    cases = []
    for m, p in km.HOST_SHAPES + ((4, 3), (8, 3)):
        points = km.point_cases(5, p, seed=m)                      # 0, 1, r - 1 and 42 among them
        for name, sets in sorted(km.mask_families(m, p, seed=m + p).items()):
            cases.append((points, sets, rng.randrange(R_MOD), rng.choice([0, points[0], rng.randrange(R_MOD)]),
                          [[rng.randrange(R_MOD) for _ in range(p)] for _ in range(m)]))
    text = "%d\n" % len(cases)
    for points, sets, gamma, u, ys in cases:
        text += "%d %d %x %x\n%s\n%s\n%s\n" % (len(sets), len(points), gamma, u, " ".join("%x" % t for t in points), " ".join("%d" % s for s in sets),
                                             " ".join("%x" % y for row in ys for y in row))
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[-1] == ["kzg_multi_plan_check:", "ok"]
    at = 0
    for points, sets, gamma, u, ys in cases:
        want_w = km.weights(points, sets)
        want_m = km.matrix(points, sets, gamma)
        want_c, want_z = km.c_values(points, sets, gamma, u)
        assert lines[at][0] == "sets" and int(lines[at][1]) == 0                       # well-formed
        assert [int(x, 16) for x in lines[at + 1][1:]] == [x for row in want_w for x in row]
        assert [int(x, 16) for x in lines[at + 2][1:]] == [x for row in want_m for x in row]
        assert [int(x, 16) for x in lines[at + 3][1:]] == want_c + [want_z]
        assert [int(x, 16) for x in lines[at + 4][1:]] == [km.r_at(points, s, row, u) for s, row in zip(sets, ys)]
        at += 5
