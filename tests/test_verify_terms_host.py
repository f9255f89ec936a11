"""plk_verify_terms (pure CPU): the flattened form of the verifier's two pairing arguments — one scalar per distinct point — against the
verifier itself.  For the golden vk.bin / proof.bin and every tampering case of the verifier's own tests the 23 + 2 terms are summed with
the ORACLE's curve arithmetic and the two sums go to plk_pairing_check; where the scalar checks already settle the verdict, early = False is
the verdict.  In every case the result must be what plk_verify says.  This pins the flattening that plk_verify_many runs, without a GPU."""
import os

import numpy as np
import pytest

from oracle import oracle_lib as ol
from oracle import plonk_oracle as po

R_MOD = po.R_MOD


@pytest.fixture(scope="module")
def vk_proof(golden_dir):
    return (open(os.path.join(golden_dir, "vk.bin"), "rb").read(), open(os.path.join(golden_dir, "proof.bin"), "rb").read())


def _with(proof, **changes):
    P = po.read_proof(proof)
    for k, v in changes.items():
        setattr(P, k, v(getattr(P, k)))
    return po.write_proof(P)


def tampering_cases(proof):
    """name -> (tampered proof bytes, kind): kind "scalar" breaks the equation at z, "commitment" reaches the pairing"""
    bump = lambda x: (x + 1) % R_MOD
    bump_first = lambda xs: [bump(xs[0])] + list(xs[1:])
    swap01 = lambda xs: [xs[1], xs[0]] + list(xs[2:])
    P0 = po.read_proof(proof)
    scalars = {"inputs": bump_first, "wire_values_at_z": bump_first, "wire_values_at_z_omega": bump_first,
               "permutation_polynomials_at_z": bump_first, "grand_product_at_z_omega": bump,
               "quotient_polynomial_at_z": bump, "linearization_polynomial_at_z": bump}
    commitments = {"wire_commitments": swap01, "quotient_poly_commitments": swap01,
                   "grand_product_commitment": lambda c: P0.wire_commitments[0],
                   "opening_at_z_proof": lambda c: P0.opening_at_z_omega_proof,
                   "opening_at_z_omega_proof": lambda c: P0.opening_at_z_proof}
    out = {}
    for kind, cases in (("scalar", scalars), ("commitment", commitments)):
        for field, change in cases.items():
            out[field] = (_with(proof, **{field: change}), kind)
    return out


def verdict_from_terms(vk, proof, strict=False):
    import plonkit_amd as pa
    pts, sc, early = pa.verify_terms(vk, proof, strict)
    if not early:
        assert not pts.any() and not sc.any()
        return False, early
    ks = ol.fr_ints(sc)
    inf = np.zeros(8, dtype=np.uint64)
    pg, px = inf, inf
    for k in range(23):
        pg = ol.g1_add(pg, ol.g1_mul(pts[k], ks[k]))
    for k in (23, 24):
        px = ol.g1_add(px, ol.g1_mul(pts[k], ks[k]))
    return pa.pairing_check(pg, vk[-256:-128], px, vk[-128:]), early


def test_golden_proof_through_the_terms(vk_proof):
    import plonkit_amd as pa
    vk, proof = vk_proof
    ok, early = verdict_from_terms(vk, proof)
    assert early and ok and pa.verify(vk, proof)
    pts, sc, _ = pa.verify_terms(vk, proof)
    assert ol.g1_to_ints(pts[22]) == (1, 2)                          # the generator
    assert (pts[23] == pts[20]).all() and (pts[24] == pts[21]).all()
    assert ol.fr_ints(sc)[23] == R_MOD - 1


def test_every_tampering_case_matches_verify(vk_proof):
    import plonkit_amd as pa
    vk, proof = vk_proof
    for field, (bad, kind) in tampering_cases(proof).items():
        assert bad != proof, field
        ok, early = verdict_from_terms(vk, bad)
        assert ok == pa.verify(vk, bad) == False, field
        # what the transcript absorbs before z moves every challenge, so the equation at z names it (early = False is the verdict);
        # d(z omega) and the two opening proofs are not in that equation: only the pairing can say
        assert early == (field in ("wire_values_at_z_omega", "opening_at_z_proof", "opening_at_z_omega_proof")), (field, kind)


def test_wrong_keys_and_refusals(vk_proof):
    import plonkit_amd as pa
    vk, proof = vk_proof
    V = po.read_vk(vk)
    V.permutation_commitments = [V.permutation_commitments[1], V.permutation_commitments[0]] + list(V.permutation_commitments[2:])
    for other_vk in (po.write_vk(V), vk[:-256] + vk[-128:] + vk[-256:-128]):
        ok, _ = verdict_from_terms(other_vk, proof)
        assert ok == pa.verify(other_vk, proof) == False
    for bad_vk, bad_proof, words in ((vk[:-1], proof, "malformed verification key"), (vk, proof[:-1], "malformed proof"),
                                     (vk, proof + b"\0", "malformed proof"), (b"", proof, "malformed verification key")):
        with pytest.raises(pa.PlkError, match=words) as e:
            pa.verify_terms(bad_vk, bad_proof)
        assert e.value.code == 1
        with pytest.raises(pa.PlkError, match=words):
            pa.verify(bad_vk, bad_proof)
    # another input count: a verdict, settled early
    P = po.read_proof(proof)
    P.inputs = list(P.inputs) + [5]
    more = po.write_proof(P)
    assert pa.verify_terms(vk, more)[2] is False and not pa.verify(vk, more)
