"""-m "not gpu": plk_kzg_verify (kzg.hip; pure CPU) on the reference's own tests/golden/setup_2pow10.key (tau = 42) and its G2 section.
The openings are built by the oracle alone: po.commit of the polynomials and of the quotient that the Python-integer model
(tests/gen/kzg_cases.py) divides out — no product code makes what the product code checks."""
import os
import random

import numpy as np
import pytest

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import Q_MOD, R_MOD
from tests.gen import kzg_cases as kc

ERR_ARG = 1
DEG = 24                                                         # coefficients per polynomial


@pytest.fixture(scope="module")
def pa():
    import plonkit_amd
    return plonkit_amd


@pytest.fixture(scope="module")
def g2(golden_dir):
    return open(os.path.join(golden_dir, "setup_2pow10.key"), "rb").read()[-256:]


def _opening(crs, polys, z, v):
    """(commitments [count, 8], evals [count, 4], proof [8]) of the polynomials (lists of canonical ints) at z, combined by powers of v"""
    cms = np.stack([po.commit(crs, ol.fr_vec(p)) for p in polys])
    ys = [kc.horner(p, z) for p in polys]
    F = [sum(pow(v, j, R_MOD) * p[i] for j, p in enumerate(polys)) % R_MOD for i in range(len(polys[0]))]
    proof = po.commit(crs, ol.fr_vec(kc.divide_by_linear(F, z)))
    return cms, ol.fr_vec(ys), proof


@pytest.fixture(scope="module")
def openings(golden_crs):
    rng = random.Random(20261020)
    out = {}
    for count in (1, 3, 8):
        polys = [[rng.randrange(R_MOD) for _ in range(DEG)] for _ in range(count)]
        z, v = rng.randrange(R_MOD), rng.randrange(R_MOD)
        out[count] = (z, v) + _opening(golden_crs, polys, z, v)
    return out


@pytest.mark.parametrize("count", [1, 3, 8])
def test_valid_openings(pa, g2, openings, count):
    z, v, cms, ys, proof = openings[count]
    assert pa.kzg_verify(cms, ol.fr_mont(z), ys, proof, g2, v=ol.fr_mont(v)) is True


def test_one_polynomial_needs_no_v(pa, g2, openings):
    z, v, cms, ys, proof = openings[1]
    assert pa.kzg_verify(cms, ol.fr_mont(z), ys, proof, g2) is True
    assert pa.kzg_verify(cms, ol.fr_mont(z), ys, proof, g2, v=ol.fr_mont(12345)) is True      # v^0 = 1 whatever v is


def test_several_polynomials_need_v(pa, g2, openings):
    z, v, cms, ys, proof = openings[3]
    with pytest.raises(pa.PlkError) as e:
        pa.kzg_verify(cms, ol.fr_mont(z), ys, proof, g2)
    assert e.value.code == ERR_ARG


# (v does not enter the opening of ONE polynomial — v^0 = 1, test_one_polynomial_needs_no_v — so there is no (1, "v") case)
@pytest.mark.parametrize("count,what", [(c, w) for c in (1, 3, 8) for w in ("z", "eval", "v", "proof", "commitment") if (c, w) != (1, "v")])
def test_single_tampering_is_invalid(pa, g2, openings, count, what):
    z, v, cms, ys, proof = openings[count]
    cms, ys = cms.copy(), ys.copy()
    if what == "z":
        z = (z + 1) % R_MOD
    elif what == "eval":
        ys[count - 1] = ol.fr_mont(ol.fr_ints(ys[count - 1:count])[0] + 1)
    elif what == "v":
        v = (v + 1) % R_MOD
    elif what == "proof":
        proof = ol.g1_add(proof, ol.g1_generator())
    else:
        cms[count // 2] = ol.g1_add(cms[count // 2], ol.g1_generator())
    assert pa.kzg_verify(cms, ol.fr_mont(z), ys, proof, g2, v=ol.fr_mont(v)) is False


def test_zero_and_constant_polynomials(pa, g2, golden_crs):
    inf = np.zeros(8, dtype=np.uint64)
    z = 0x1234567
    # the zero polynomial: commitment and proof are both infinity
    assert pa.kzg_verify(inf[None], ol.fr_mont(z), ol.fr_vec([0]), inf, g2) is True
    assert pa.kzg_verify(inf[None], ol.fr_mont(z), ol.fr_vec([1]), inf, g2) is False
    # a constant: the proof is infinity
    c = po.commit(golden_crs, ol.fr_vec([7]))
    assert np.array_equal(c, ol.g1_mul(ol.g1_generator(), 7))
    assert pa.kzg_verify(c[None], ol.fr_mont(z), ol.fr_vec([7]), inf, g2) is True
    assert pa.kzg_verify(c[None], ol.fr_mont(z), ol.fr_vec([8]), inf, g2) is False
    # zero among others
    cms, ys, proof = _opening(golden_crs, [[5, 6, 7], [0, 0, 0]], z, 99)
    assert not cms[1].any()
    assert pa.kzg_verify(cms, ol.fr_mont(z), ys, proof, g2, v=ol.fr_mont(99)) is True


def test_z_zero_and_extreme_scalars(pa, g2, golden_crs):
    for z, v in ((0, 1), (R_MOD - 1, R_MOD - 1), (1, 0)):
        cms, ys, proof = _opening(golden_crs, [[1, 2, 3, R_MOD - 1], [R_MOD - 1] * 4], z, v)
        assert pa.kzg_verify(cms, ol.fr_mont(z), ys, proof, g2, v=ol.fr_mont(v)) is True, (z, v)


def _refused(pa, *args, **kw):
    with pytest.raises(pa.PlkError) as e:
        pa.kzg_verify(*args, **kw)
    assert e.value.code == ERR_ARG, e.value
    return str(e.value)


def test_malformed_inputs_are_err_arg(pa, g2, openings):
    z, v, cms, ys, proof = openings[3]
    zm, vm = ol.fr_mont(z), ol.fr_mont(v)
    off = cms.copy(); off[1][4] ^= np.uint64(1)                   # y moved: off the curve
    assert "commitment 1" in _refused(pa, off, zm, ys, proof, g2, v=vm)
    badp = proof.copy(); badp[0] ^= np.uint64(1)
    assert "proof" in _refused(pa, cms, zm, ys, badp, g2, v=vm)
    big = cms.copy(); big[0][:4] = ol.int_to_limbs(Q_MOD)         # x = q: not a coordinate
    _refused(pa, big, zm, ys, proof, g2, v=vm)
    r_limbs = ol.int_to_limbs(R_MOD)
    _refused(pa, cms, r_limbs, ys, proof, g2, v=vm)               # z = r
    _refused(pa, cms, zm, ys, proof, g2, v=r_limbs)               # v = r
    e = ys.copy(); e[2] = ol.int_to_limbs((1 << 256) - 1)
    _refused(pa, cms, zm, e, proof, g2, v=vm)
    assert _refused(pa, np.zeros((9, 8), dtype=np.uint64), zm, np.zeros((9, 4), dtype=np.uint64), proof, g2, v=vm)   # count > 8


def test_g2_refusals_are_plk_pairing_checks(pa, g2, openings):
    """a G2 point that is not on the twist (and so not in the subgroup) is refused with plk_pairing_check's own words, whichever of the two it is"""
    z, v, cms, ys, proof = openings[1]
    for at in (127, 255):
        bad = bytearray(g2); bad[at] ^= 1
        with pytest.raises(pa.PlkError) as mine:
            pa.kzg_verify(cms, ol.fr_mont(z), ys, proof, bytes(bad))
        with pytest.raises(pa.PlkError) as theirs:
            pa.pairing_check(proof, bytes(bad[:128]), proof, bytes(bad[128:]))
        assert mine.value.code == theirs.value.code == ERR_ARG
        assert str(mine.value) == str(theirs.value) and "not on the twist" in str(mine.value)
