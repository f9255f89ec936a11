"""The host verifier (plk_verify_ex) and the flattening that plk_verify_many runs (plk_verify_terms) on FORGED proofs (pure CPU).

tests/gen/forged_proofs.py builds, from a key's trapdoor, proofs that verify although no prover made them: points at infinity everywhere,
zero scalars, consecutive terms that coincide or cancel, N = 2 and N = 2^28, 0 / 1 / 9 / 300 public inputs, trapdoors 1, r - 1, 5 and a
random one, and G2 points at infinity.  A "valid" verdict needs every one of the 25 products and both sums exact, which the tamperings of
honest proofs (expected "invalid") never ask.  For every case:
  * plk_verify_ex says what the oracle says (forge_record has asserted oracle == the forger's own logarithms);
  * the 25 terms of plk_verify_terms, summed with the oracle's curve arithmetic, are EXACTLY the points the forger's logarithms name,
    and plk_pairing_check on the two sums gives the same verdict.
Where a G2 point is at infinity the oracle has no model: the verdict is the closed form "pg is O" / "px is O"."""
import random

import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD
from tests.gen import forged_proofs as fp

EDGE = fp.edge_cases()
BROKEN = fp.broken_cases()
CASES = dict(EDGE, **BROKEN)
O = np.zeros(8, dtype=np.uint64)


def term_products(vk, proof):
    """the 25 products s_k P_k of plk_verify_terms, by the oracle"""
    import plonkit_amd as pa
    pts, sc, early = pa.verify_terms(vk, proof, False)
    assert early, "a forged proof keeps the equation at z: it must reach the group arithmetic"
    ks = ol.fr_ints(sc)
    return [O if (ks[k] == 0 or ol.g1_is_inf(pts[k])) else ol.g1_mul(pts[k], ks[k]) for k in range(25)], pts, ks


def partial_sums(prods, lo, hi):
    out, acc = [], O
    for k in range(lo, hi):
        acc = ol.g1_add(acc, prods[k])
        out.append(acc)
    return out


def check_against_logs(f, g2=None):
    """-> (verdict of plk_verify_ex, products, points, scalars) after the exact comparisons"""
    import plonkit_amd as pa
    prods, pts, ks = term_products(f.vk, f.proof)
    pg, px = partial_sums(prods, 0, 23)[-1], partial_sums(prods, 23, 25)[-1]
    assert (pg == fp.g1_of(f.pg)).all() and (px == fp.g1_of(f.px)).all()
    host = pa.verify(f.vk, f.proof, strict_inputs=False)
    assert pa.pairing_check(pg, f.vk[-256:-128], px, f.vk[-128:]) == host
    return host, prods, pts, ks


@pytest.mark.parametrize("name", sorted(CASES))
def test_forged_case_matches_the_oracle(name):
    f = fp.forge_record(**CASES[name])
    assert f.valid == (name in EDGE)
    host, _, _, _ = check_against_logs(f)
    assert host == f.valid


def test_the_constructions_reach_what_they_name():
    """the special cases are special in the terms themselves: identity products, equal and opposite neighbours, sums through O"""
    neg = ol.g1_neg
    same = lambda a, b: bool((a == b).all())
    inf = ol.g1_is_inf

    _, prods, pts, ks = check_against_logs(fp.forge_record(**EDGE["all_infinity_N2"]))
    assert all(inf(pts[k]) for k in range(20)) and all(inf(prods[k]) for k in range(20)) and not inf(prods[22])
    _, prods, pts, ks = check_against_logs(fp.forge_record(**EDGE["all_infinity_zero_evaluations_N2"]))
    assert all(ks[k] == 0 for k in (0, 1, 2, 3, 4, 6, 10))

    _, prods, _, ks = check_against_logs(fp.forge_record(**EDGE["equal_key_doubling_at_step_1"]))
    assert ks[0] == ks[1] and same(prods[0], prods[1]) and not inf(prods[0]) and ks[2] == ks[3] == 0
    _, prods, _, ks = check_against_logs(fp.forge_record(**EDGE["equal_key_cancellation_at_step_1"]))
    assert same(prods[0], neg(prods[1])) and not inf(prods[0]) and inf(partial_sums(prods, 0, 23)[1]) and not inf(prods[4])
    _, prods, _, ks = check_against_logs(fp.forge_record(**EDGE["equal_key_doubling_at_step_5"]))
    s = partial_sums(prods, 0, 23)
    assert all(inf(prods[k]) for k in (0, 1, 2, 4)) and inf(s[2]) and same(s[4], prods[5]) and not inf(prods[5]) and ks[3] == ks[5]
    _, prods, _, ks = check_against_logs(fp.forge_record(**EDGE["equal_key_cancellation_at_step_5"]))
    s = partial_sums(prods, 0, 23)
    assert same(s[4], neg(prods[5])) and inf(s[5]) and not inf(prods[5]) and not inf(s[-1])

    for name, rel in (("other_representation_doubling", lambda a, b: same(a, b)), ("other_representation_cancellation", lambda a, b: same(a, neg(b)))):
        _, prods, pts, ks = check_against_logs(fp.forge_record(**EDGE[name]))
        assert rel(prods[0], prods[1]) and not same(pts[0], pts[1]) and ks[0] != ks[1] and not inf(prods[0])

    _, prods, pts, ks = check_against_logs(fp.forge_record(**EDGE["all_generator_unit_evaluations"]))
    assert all(same(pts[k], pts[22]) for k in range(20))
    _, prods, pts, ks = check_against_logs(fp.forge_record(**EDGE["no_opening_at_z_omega"]))
    assert inf(pts[21]) and inf(pts[24]) and inf(pts[15]) and inf(pts[14]) and ks[21] != 0
    _, prods, pts, ks = check_against_logs(fp.forge_record(**EDGE["evaluations_r_minus_1_N2^28"]))
    assert ks[23] == R_MOD - 1

    for name in BROKEN:
        f = fp.forge_record(**BROKEN[name])
        assert (f.pg == 0) == name.startswith("pg_inf") and (f.px == 0) == name.startswith("px_inf")


def test_twist_arithmetic_and_other_trapdoors():
    """keys of other trapdoors: tau G2 from the plain-integer twist code, which reproduces the golden 42 G2 before anything uses it"""
    import plonkit_amd as pa
    g, g42 = fp.golden_g2()
    assert g + g42 == pa.crs42_g2_bytes() == fp.g2_pair(42)
    assert fp.g2_mul_bytes(g, 42) == g42 and fp.g2_mul_bytes(g, R_MOD - 1) == fp.g2_neg_bytes(g) and fp.g2_mul_bytes(g, R_MOD) == fp.G2_INF
    assert fp.g2_neg_bytes(fp.g2_neg_bytes(g42)) == g42 and fp.g2_neg_bytes(g42) != g42
    rng = random.Random(77)
    tau = rng.randrange(R_MOD)
    args = fp.random_args(rng, 15, 1)
    for variant, want in ((None, True), ("plus_g", False), ("px_inf", False)):
        f = fp.forge_record(**dict(args, tau=tau, variant=variant))
        assert f.valid == want and check_against_logs(f)[0] == want
    # the proof of one trapdoor under the key of another
    a, b = fp.forge_record(**dict(args, tau=5)), fp.forge_record(**dict(args, tau=tau))
    assert a.vk[:-128] == b.vk[:-128] and a.vk != b.vk
    assert pa.verify(a.vk, a.proof) and pa.verify(b.vk, b.proof) and not pa.verify(a.vk, b.proof) and not pa.verify(b.vk, a.proof)


G2_WITH_INFINITY = {"g2[0]": lambda g: fp.G2_INF + g[128:], "g2[1]": lambda g: g[:128] + fp.G2_INF, "both": lambda g: fp.G2_INF * 2}


@pytest.mark.parametrize("which", sorted(G2_WITH_INFINITY))
def test_g2_at_infinity_is_the_closed_form(which):
    """e(., O) = 1: the verdict is "px is O" when g2[0] is at infinity, "pg is O" when g2[1] is, and valid when both are"""
    rng = random.Random(99)
    g2 = G2_WITH_INFINITY[which](fp.g2_pair(42))
    base = fp.random_args(rng, 1, 1)
    want = {"g2[0]": {None: False, "px_inf": True, "pg_inf": False}, "g2[1]": {None: False, "px_inf": False, "pg_inf": True},
            "both": {None: True, "px_inf": True, "pg_inf": True}}[which]
    for variant in (None, "px_inf", "pg_inf"):
        f = fp.forge_record(**dict(fp.no_wzw(base) if variant == "pg_inf" else base, variant=variant, g2=g2))
        assert f.valid is None and fp.g2_inf_verdict(f, g2) == want[variant]
        host, _, _, _ = check_against_logs(f)
        assert host == want[variant], (which, variant)
