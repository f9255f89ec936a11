"""plk_vk_load / plk_verify_many / plk_pairing_check_many_dev on the GPU: every proof of a batch verified exactly and on its own, verdict i =
what plk_verify_ex says about proof i (1 valid, 0 invalid, 2 malformed).  Proofs come from the synthetic generator (about 200 gates, one R1CS,
a witness per proof) against one setup and a tau = 42 key of 2^10 points; the cost of verifying does not depend on the domain.  The host
verdicts are computed once per distinct proof and shared between the tests."""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import R_MOD

pytestmark = pytest.mark.gpu

ERR_ARG = 1
VALID, INVALID, MALFORMED = 1, 0, 2


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


class Batch:
    """200 proofs of one circuit, its key, a proof of another circuit, and the host's verdict per proof (cached)"""

    def __init__(self, ctx):
        import plonkit_amd as pa
        ctx.srs_generate(1 << 10, 0, 42)
        ctx.srs_lagrange_clear()
        first = pa.Circuit.synthetic_ex(200, 4242, 1)
        self.setup = pa.SetupForProver(ctx, first)
        self.vk = self.setup.verification_key_bytes(pa.crs42_g2_bytes())
        self.proofs = []
        for k in range(1, 201):
            c = first if k == 1 else pa.Circuit.synthetic_ex(200, 4242, k)
            self.proofs.append(self.setup.prove(c))
            c.close()
        assert len(set(self.proofs)) == 200
        other = pa.Circuit.synthetic_ex(200, 777, 1)
        s2 = pa.SetupForProver(ctx, other)
        self.foreign = s2.prove(other)
        s2.close(); other.close()
        self._host = {}

    def host(self, proof):
        """plk_verify_ex on the host: 1 / 0, or 2 where it returns PLK_ERR_ARG"""
        import plonkit_amd as pa
        if proof not in self._host:
            try:
                self._host[proof] = VALID if pa.verify(self.vk, proof, strict_inputs=False) else INVALID
            except pa.PlkError as e:
                assert e.code == ERR_ARG
                self._host[proof] = MALFORMED
        return self._host[proof]


@pytest.fixture(scope="module")
def batch(ctx):
    return Batch(ctx)


@pytest.fixture(scope="module")
def key(ctx, batch):
    import plonkit_amd as pa
    k = pa.VerificationKey(ctx, batch.vk, strict_inputs=False)
    yield k
    k.close()


def _with(proof, **changes):
    P = po.read_proof(proof)
    for k, v in changes.items():
        setattr(P, k, v(getattr(P, k)))
    return po.write_proof(P)


def tamperings(proof):
    """one tampering of each kind: every scalar moved by one, every commitment replaced by another curve point"""
    bump = lambda x: (x + 1) % R_MOD
    bump_first = lambda xs: [bump(xs[0])] + list(xs[1:])
    swap01 = lambda xs: [xs[1], xs[0]] + list(xs[2:])
    P0 = po.read_proof(proof)
    cases = {"inputs": bump_first, "wire_values_at_z": bump_first, "wire_values_at_z_omega": bump_first,
             "permutation_polynomials_at_z": bump_first, "grand_product_at_z_omega": bump,
             "quotient_polynomial_at_z": bump, "linearization_polynomial_at_z": bump,
             "wire_commitments": swap01, "quotient_poly_commitments": swap01,
             "grand_product_commitment": lambda c: P0.wire_commitments[0],
             "opening_at_z_proof": lambda c: P0.opening_at_z_omega_proof,
             "opening_at_z_omega_proof": lambda c: P0.opening_at_z_proof}
    return [_with(proof, **{f: c}) for f, c in cases.items()]


# ---------------------------------------------------------------------------------------------- the pairing kernel on its own
@pytest.fixture(scope="module")
def pairs():
    """130 + 4 pairs (A, B) for {G2, 42 G2}: e(A, Q0) e(B, Q1) = 1 iff A + 42 B = O.  Two thirds true (B = b G, A = -42 b G), one third off by one"""
    rng = random.Random(20261018)
    G = ol.g1_generator()
    a, b = [], []
    for i in range(130):
        k = rng.randrange(1, R_MOD)
        b.append(ol.g1_mul(G, k))
        a.append(ol.g1_neg(ol.g1_mul(G, (42 * k + (1 if i % 3 == 2 else 0)) % R_MOD)))
    O = np.zeros(8, dtype=np.uint64)
    special = [(O, O), (O, b[0]), (a[0], O), (ol.g1_from_ints(1, 3), b[1])]          # 1, 0, 0, and (1, 3) is not on the curve: 2
    return np.array(a), np.array(b), special


def _host_pairing(a, b, g2):
    import plonkit_amd as pa
    try:
        return VALID if pa.pairing_check(a, g2[:128], b, g2[128:]) else INVALID
    except pa.PlkError as e:
        assert e.code == ERR_ARG
        return MALFORMED


@pytest.fixture(scope="module")
def pair_verdicts(pairs):
    import plonkit_amd as pa
    a, b, special = pairs
    g2 = pa.crs42_g2_bytes()
    return [_host_pairing(a[i], b[i], g2) for i in range(130)], [_host_pairing(x, y, g2) for x, y in special]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_pairing_check_many_dev_against_closed_forms(ctx, pairs, pair_verdicts, n):
    import torch
    import plonkit_amd as pa
    a, b, special = pairs
    want_main, want_special = pair_verdicts
    assert want_special == [1, 0, 0, 2] and want_main[:3] == [1, 1, 0]
    A = np.concatenate([a[:n], np.array([s[0] for s in special])])
    B = np.concatenate([b[:n], np.array([s[1] for s in special])])
    total = n + len(special)
    dA = torch.from_numpy(A.astype(np.int64)).cuda(); dB = torch.from_numpy(B.astype(np.int64)).cuda()
    out = torch.full((total + 16,), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.pairing_check_many_dev(dA.data_ptr(), dB.data_ptr(), total, pa.crs42_g2_bytes(), out.data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    assert got[:total].tolist() == want_main[:n] + want_special
    assert (got[total:] == 77).all()                                 # nothing behind the last verdict byte is written
    with pytest.raises(pa.PlkError) as e:
        ctx.pairing_check_many_dev(dA.data_ptr() + 8, dB.data_ptr(), total, pa.crs42_g2_bytes(), out.data_ptr())
    assert e.value.code == ERR_ARG
    bad_g2 = bytearray(pa.crs42_g2_bytes()); bad_g2[127] ^= 1
    with pytest.raises(pa.PlkError, match="G2 point not on the twist"):
        ctx.pairing_check_many_dev(dA.data_ptr(), dB.data_ptr(), total, bytes(bad_g2), out.data_ptr())


# ---------------------------------------------------------------------------------------------- whole proofs
def test_golden_proof_alone(ctx, golden_dir):
    import plonkit_amd as pa
    vk, proof = (open(os.path.join(golden_dir, f), "rb").read() for f in ("vk.bin", "proof.bin"))
    k = pa.VerificationKey(ctx, vk)
    v = k.verify_many([proof])
    assert v.dtype == np.uint8 and v.tolist() == [1] and k.first_bad is None
    assert pa.verify(vk, proof) and po.verify(po.read_vk(vk), po.read_proof(proof))
    assert k.verify_many([proof[:-1]]).tolist() == [2] and k.first_bad == 0
    k.close()
    for bad in (vk[:-1], b""):
        with pytest.raises(pa.PlkError, match="malformed verification key"):
            pa.VerificationKey(ctx, bad)


@pytest.mark.parametrize("count", [65, 200])
def test_mixed_batch_matches_verify_ex_per_proof(ctx, batch, key, count):
    rng = random.Random(1000 + count)
    proofs = list(batch.proofs[:count])
    bad = tamperings(proofs[3]) + [proofs[5][:-7], batch.foreign]
    for i, b in zip(rng.sample(range(count), len(bad)), bad):
        proofs[i] = b
    want = [batch.host(p) for p in proofs]
    assert want.count(MALFORMED) == 1 and want.count(INVALID) == len(bad) - 1 and want.count(VALID) == count - len(bad)
    got = key.verify_many(proofs)
    assert got.tolist() == want
    assert key.first_bad == min(i for i, w in enumerate(want) if w != VALID)
    vk = po.read_vk(batch.vk)
    for i in rng.sample(range(count), 5):
        if want[i] != MALFORMED:
            assert po.verify(vk, po.read_proof(proofs[i])) == bool(want[i]), i


def test_all_valid_all_invalid_and_empty(ctx, batch, key):
    import ctypes
    import plonkit_amd as pa
    good = batch.proofs[:70]
    assert all(batch.host(p) == VALID for p in good)
    assert key.verify_many(good).tolist() == [1] * 70 and key.first_bad is None
    worse = [_with(p, opening_at_z_proof=lambda c, P=po.read_proof(p): P.opening_at_z_omega_proof) for p in batch.proofs[:3]]   # these reach the pairing
    worse += [_with(p, quotient_polynomial_at_z=lambda x: (x + 1) % R_MOD) for p in batch.proofs[3:6]]
    assert all(batch.host(p) == INVALID for p in worse)
    assert key.verify_many(worse).tolist() == [0] * 6 and key.first_bad == 0
    assert key.verify_many([]).tolist() == [] and key.first_bad is None
    fb = ctypes.c_uint64(5)
    assert pa.lib().plk_verify_many(ctx._h, key._h, None, None, ctypes.c_uint64(0), ctypes.create_string_buffer(1), ctypes.byref(fb)) == 0 and fb.value == 2 ** 64 - 1
    assert pa.lib().plk_verify_many(ctx._h, key._h, None, None, ctypes.c_uint64(1), ctypes.create_string_buffer(1), ctypes.byref(fb)) == ERR_ARG
    assert pa.lib().plk_verify_many(ctx._h, None, None, None, ctypes.c_uint64(0), ctypes.create_string_buffer(1), ctypes.byref(fb)) == ERR_ARG


def test_one_key_from_two_contexts(ctx, batch, key):
    import plonkit_amd as pa
    other = pa.Context(0)
    proofs = batch.proofs[:9] + [batch.foreign]
    want = [batch.host(p) for p in proofs]
    assert key.verify_many(proofs, ctx=other).tolist() == want
    assert key.verify_many(proofs).tolist() == want
    other.close()


def test_strict_inputs_on_a_zero_input_key(ctx, golden_crs):
    """a circuit without public inputs (from the oracle, on the CPU): valid by default, refused under the strict rule, as plk_verify_ex"""
    import plonkit_amd as pa
    u, v = 3, 5
    wit = [1, u, v, u * v % R_MOD]
    cons = [({"1": "1"}, {"2": "1"}, {"3": "1"})]
    for _ in range(4):
        wit.append(wit[-1] * v % R_MOD)
        cons.append(({str(len(wit) - 2): "1"}, {"2": "1"}, {str(len(wit) - 1): "1"}))
    js = {"n8": 32, "prime": str(R_MOD), "nVars": len(wit), "nOutputs": 0, "nPubInputs": 0, "nPrvInputs": 2,
          "nLabels": len(wit), "nConstraints": len(cons), "constraints": [list(c) for c in cons]}
    r1cs = po.load_r1cs_json(js)
    S = po.setup(r1cs)
    proof = po.write_proof(po.prove(r1cs, wit, golden_crs, S))
    vk = po.write_vk(po.make_verification_key(S, golden_crs))
    assert len(po.read_proof(proof).inputs) == 0
    for strict in (False, True):
        k = pa.VerificationKey(ctx, vk, strict_inputs=strict)
        assert k.verify_many([proof, proof]).tolist() == [int(pa.verify(vk, proof, strict_inputs=strict))] * 2 == [0 if strict else 1] * 2
        k.close()


def test_commitment_in_flight_is_refused(ctx, batch, key):
    import torch
    import plonkit_amd as pa
    sc = torch.from_numpy(ol.fr_vec(list(range(1, 65))).astype(np.int64)).cuda()
    torch.cuda.synchronize()
    ctx.msm_enqueue_dev(sc.data_ptr(), 64)
    with pytest.raises(pa.PlkError, match="in flight") as e:
        key.verify_many(batch.proofs[:2])
    assert e.value.code == ERR_ARG
    ctx.msm_finish()
    assert key.verify_many(batch.proofs[:2]).tolist() == [1, 1]


def test_no_allocation_once_the_arena_has_grown(ctx, batch, key):
    import torch
    proofs = batch.proofs[:120]
    key.verify_many(proofs)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    key.verify_many(proofs)
    key.verify_many(proofs[:50])
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == before


def test_cli_verify_many(batch, tmp_path):
    import plonkit_amd as pa
    cli = os.path.join(os.path.dirname(pa.lib_path()), "plonkit")
    vkp = tmp_path / "vk.bin"; vkp.write_bytes(batch.vk)
    files = [tmp_path / ("p%d.bin" % i) for i in range(3)]
    files[0].write_bytes(batch.proofs[0]); files[2].write_bytes(batch.proofs[2])
    files[1].write_bytes(_with(batch.proofs[1], opening_at_z_proof=lambda c: po.read_proof(batch.proofs[1]).opening_at_z_omega_proof))
    r = subprocess.run(["timeout", "-k", "10", "120", cli, "verify-many", "-v", str(vkp)] + [str(f) for f in files], capture_output=True, text=True, timeout=150)
    assert r.returncode == 144, r.stderr
    assert r.stdout.splitlines() == ["%s: %s" % (f, w) for f, w in zip(files, ("valid", "invalid", "valid"))]
    files[1].write_bytes(batch.proofs[1][:40])
    r = subprocess.run(["timeout", "-k", "10", "120", cli, "verify-many", "-v", str(vkp)] + [str(f) for f in files], capture_output=True, text=True, timeout=150)
    assert r.returncode == 144 and r.stdout.splitlines()[1] == "%s: malformed" % files[1]
    r = subprocess.run(["timeout", "-k", "10", "120", cli, "verify-many", "-v", str(vkp), str(files[0]), str(files[2])], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and r.stdout.count(": valid") == 2
    usage = subprocess.run([cli], capture_output=True, text=True)
    assert "verify-many -v <vk> <proof>..." in usage.stderr and "check-key" in usage.stderr
