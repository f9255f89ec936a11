"""plk_verify_many / plk_pairing_check_many_dev on FORGED proofs: the glue of verify_many.hip where the expected verdict is "valid".

A "valid" verdict needs all 25 products, both sums, the shared inversion and the pairing exact; the suite's other valid cases are honest
proofs with generic points and scalars.  tests/gen/forged_proofs.py builds, from a key's trapdoor, proofs that verify under the oracle
(it asserts so for every one) and that put on the device what no prover does:
  vm_mul_kernel     points at infinity and scalars of exactly 0
  vm_sum_kernel     an identity first term, consecutive equal terms (the doubling branch), the same element in two XYZZ representations,
                    acc == -next with the sum continuing from the identity
  vm_affine_kernel  a sum at infinity at each of the 8 positions of an inversion group, between neighbours whose verdicts must not move
  the pairing       G2 pairs other than {G2, 42 G2}, G2 points at infinity (q_inf), the replacement of a context's cached table
  the driver        N = 2 and N = 2^28, and more than VM_CHUNK = 2^16 proofs in one call
Every expected verdict is the oracle's (or, where a G2 point is at infinity, the closed form "pg is O" / "px is O" from the forger's own
logarithms); every assertion is an exact equality."""
import random
import time

import numpy as np
import pytest

from oracle import plonk_oracle as po
from oracle.oracle_lib import R_MOD
from tests.gen import forged_proofs as fp

pytestmark = pytest.mark.gpu

VALID, INVALID, MALFORMED = 1, 0, 2
BATCH = 131            # crosses 4 proofs per inversion group, 10.24 proofs per vm_mul_kernel workgroup, 64 lanes per pairing workgroup, 128 proofs per vm_sum_kernel workgroup
ROTATIONS = (0, 1, 2, 3)
BIG = R_MOD - 1


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def _bump_t_z(proof):
    """t(z) + 1: the equation at z fails, the host settles the verdict and the proof never reaches the device"""
    P = po.read_proof(proof)
    P.quotient_polynomial_at_z = (P.quotient_polynomial_at_z + 1) % R_MOD
    return po.write_proof(P)


def _verdict(f):
    assert f.valid is not None
    return VALID if f.valid else INVALID


# ---------------------------------------------------------------------------------------------- the key families
def _family(name):
    """-> (key logarithms, n, number of inputs, [the family's own valid constructions: rng -> changes to random arguments])"""
    rng = random.Random("key of " + name)
    fr = lambda r: r.randrange(R_MOD)
    if name == "random":
        key = [rng.randrange(R_MOD) for _ in range(11)]
        own = [lambda r: {}, lambda r: dict(wz=[BIG] * 4, wzw=BIG, z_zw=BIG, sz=[BIG] * 3, r_z=BIG, inputs=[BIG, BIG]),
               lambda r: dict(wz=[0] * 4, wzw=0, sz=[0] * 3, r_z=0, inputs=[0, 0])]
        return key, (1 << 10) - 1, 2, own
    if name == "equal":                                               # all points equal: consecutive terms of the sum coincide or cancel
        def pair(sign, step):
            def change(r):
                a = fr(r)
                return dict(wz=[a, sign * a % R_MOD, 0, 0]) if step == 1 else dict(wz=[0, 0, 0, sign % R_MOD])
            return change
        return [rng.randrange(R_MOD)] * 11, 7, 1, [pair(1, 1), pair(-1, 1), pair(1, 5), pair(-1, 5), lambda r: {}]
    if name == "infinity":                                            # all points at infinity, N = 2, no inputs
        own = [lambda r: dict(wires=[0] * 4, Z=0, t=[0] * 4), lambda r: dict(wires=[0] * 4, Z=0, t=[0] * 4, wz=[0] * 4, wzw=0, z_zw=0),
               lambda r: {}, lambda r: dict(wires=[0, fr(r), 0, fr(r)], t=[0, 0, fr(r), 0])]
        return [0] * 11, 1, 0, own
    if name == "generator":                                           # the key, the proof and term 22 on the generator; N = 2^28
        on_g = dict(wires=[1] * 4, Z=1, t=[1] * 4)
        own = [lambda r: dict(on_g), lambda r: dict(on_g, wz=[1] * 4, wzw=1, z_zw=1, sz=[1] * 3, r_z=1), lambda r: {},
               lambda r: dict(on_g, wz=[fr(r), BIG, 0, 1])]
        return [1] * 11, (1 << 28) - 1, 1, own
    raise KeyError(name)


def _family_batch(name):
    """BATCH forged proofs of one key, all different, in a fixed pattern of eight:
         valid | px = O | W_z + G | valid | pg = O | W_z + G | valid with W_zw = O | valid
    so that every sum at infinity has, on each side, a neighbour that reaches the pairing — one whose verdict is "valid" and one
    whose verdict is "invalid" although the device computes it (a neighbour that came out at infinity too would pass for valid)."""
    key, n, ni, own = _family(name)
    rng = random.Random("proofs of " + name)
    out, vk = [], None
    for i in range(BATCH):
        args = fp.random_args(rng, n, ni, key=key)
        args.update(own[(i // 8 + i) % len(own)](rng))
        slot = i % 8
        if slot == 1:
            args["variant"] = "px_inf"
        elif slot in (2, 5):
            args["variant"] = "plus_g"
        elif slot == 4:
            args = dict(fp.no_wzw(args), variant="pg_inf")
        elif slot == 6:
            args = fp.no_wzw(args)
        f = fp.forge_record(**args)
        assert vk in (None, f.vk)
        vk = f.vk
        assert f.valid == (slot in (0, 3, 6, 7)) and (f.px == 0) == (slot == 1) and (f.pg == 0) == (slot == 4), (name, i)
        out.append((f.proof, _verdict(f)))
    assert len(set(p for p, _ in out)) == BATCH
    # two that the host settles: they leave the packed list that the device sees, and shift everything behind them
    out[77] = (out[76][0][:-9], MALFORMED)
    out[129] = (_bump_t_z(out[128][0]), INVALID)
    return vk, out


@pytest.mark.parametrize("name", ["random", "equal", "infinity", "generator"])
def test_family_batch_at_every_rotation(ctx, name):
    import plonkit_amd as pa
    vk, batch = _family_batch(name)
    key = pa.VerificationKey(ctx, vk, strict_inputs=False)
    try:
        for k in ROTATIONS:
            rot = batch[k:] + batch[:k]
            want = [w for _, w in rot]
            got = key.verify_many([p for p, _ in rot])
            assert got.tolist() == want, (name, k, [i for i in range(BATCH) if got[i] != want[i]])
            assert key.first_bad == min(i for i, w in enumerate(want) if w != VALID)
        good = [p for p, w in batch if w == VALID]
        assert len(good) >= 64 and key.verify_many(good).tolist() == [VALID] * len(good) and key.first_bad is None
    finally:
        key.close()


def test_two_representations_of_one_element(ctx):
    """key point 2c with scalar a/2 next to key point c with scalar a: terms 0 and 1 are the same element (or opposite ones) from two
    different computations, so their XYZZ coordinates differ where the doubling / cancellation test of the addition must still see them"""
    import plonkit_amd as pa
    rng = random.Random(5150)
    c = rng.randrange(R_MOD)
    key = [2 * c % R_MOD] + [c] * 10
    proofs, want, vk = [], [], None
    for i in range(9):
        a = rng.randrange(R_MOD)
        half = a * pow(2, -1, R_MOD) % R_MOD
        args = dict(fp.random_args(rng, 3, 1, key=key), wz=[half, a if i % 2 == 0 else R_MOD - a, 0, 0], variant="plus_g" if i % 3 == 2 else None)
        f = fp.forge_record(**args)
        vk = f.vk
        proofs.append(f.proof); want.append(_verdict(f))
    assert want == [1, 1, 0] * 3
    k = pa.VerificationKey(ctx, vk, strict_inputs=False)
    assert k.verify_many(proofs).tolist() == want and k.first_bad == 2
    k.close()


# ---------------------------------------------------------------------------------------------- one proof per call
NAMED = dict(fp.edge_cases(), **fp.broken_cases())


@pytest.mark.parametrize("name", sorted(NAMED))
def test_single_proof_calls(ctx, name):
    """every named construction alone in a call (one lane of the pairing kernel, 25 of vm_mul_kernel, an inversion group of two)"""
    import plonkit_amd as pa
    f = fp.forge_record(**NAMED[name])
    k = pa.VerificationKey(ctx, f.vk, strict_inputs=False)
    assert k.verify_many([f.proof]).tolist() == [_verdict(f)]
    assert k.first_bad == (None if f.valid else 0)
    k.close()


# ---------------------------------------------------------------------------------------------- other G2 pairs
TAUS = {"1": 1, "r_minus_1": R_MOD - 1, "small": 5, "random": random.Random(4242).randrange(R_MOD)}


@pytest.mark.parametrize("which", sorted(TAUS))
def test_keys_of_other_trapdoors(ctx, which):
    """the line table that plk_vk_load builds for a Q other than 42 G2, walked by the device; and a proof forged for tau = 42
    under that key is invalid"""
    import plonkit_amd as pa
    tau = TAUS[which]
    rng = random.Random("tau " + which)
    key = [rng.randrange(R_MOD) for _ in range(11)]
    proofs, want, vk = [], [], None
    for i in range(9):
        args = fp.random_args(rng, 15, 1, key=key)
        f = fp.forge_record(**dict(args, tau=tau, variant=(None, None, "plus_g", "px_inf")[i % 4]))
        vk = f.vk
        proofs.append(f.proof); want.append(_verdict(f))
    other = fp.forge_record(**dict(fp.random_args(rng, 15, 1, key=key), tau=42))
    assert other.vk[:-128] == vk[:-128]
    proofs.append(other.proof); want.append(INVALID)
    assert want == [1, 1, 0, 0, 1, 1, 0, 0, 1, 0]
    assert not po.verify(po.read_vk(vk), po.read_proof(other.proof), tau)
    k = pa.VerificationKey(ctx, vk, strict_inputs=False)
    assert k.verify_many(proofs).tolist() == want and k.first_bad == 2
    k.close()


G2_WITH_INFINITY = {"g2[0]": lambda g: fp.G2_INF + g[128:], "g2[1]": lambda g: g[:128] + fp.G2_INF, "both": lambda g: fp.G2_INF * 2}


@pytest.mark.parametrize("which", sorted(G2_WITH_INFINITY))
def test_keys_with_g2_at_infinity(ctx, which):
    """the q_inf bits of the table: e(., O) = 1, so the verdict is "px is O" / "pg is O" / always valid"""
    import plonkit_amd as pa
    g2 = G2_WITH_INFINITY[which](fp.g2_pair(42))
    rng = random.Random("g2 at infinity " + which)
    key = [rng.randrange(R_MOD) for _ in range(11)]
    proofs, want, vk = [], [], None
    for i in range(8):
        variant = (None, "px_inf", "pg_inf", "plus_g")[i % 4]
        args = fp.random_args(rng, 1, 1, key=key)
        f = fp.forge_record(**dict(fp.no_wzw(args) if variant == "pg_inf" else args, variant=variant, g2=g2))
        vk = f.vk
        proofs.append(f.proof); want.append(VALID if fp.g2_inf_verdict(f, g2) else INVALID)
    assert want == {"g2[0]": [0, 1, 0, 0] * 2, "g2[1]": [0, 0, 1, 0] * 2, "both": [1] * 8}[which]
    k = pa.VerificationKey(ctx, vk, strict_inputs=False)
    assert k.verify_many(proofs).tolist() == want
    k.close()


# ---------------------------------------------------------------------------------------------- the pairing kernel on its own
G2_PAIRS = dict({"tau_" + k: v for k, v in TAUS.items()}, **{"inf_" + k: None for k in G2_WITH_INFINITY})
N_PAIRS = 70                                                          # more than one 64-lane workgroup


def _g2_bytes(name):
    return fp.g2_pair(TAUS[name[4:]]) if name.startswith("tau_") else G2_WITH_INFINITY[name[4:]](fp.g2_pair(42))


def _closed_form(name, a, b):
    """e(aG, Q0) e(bG, Q1) == 1 from the logarithms: a + tau b == 0, or what is left of it when a Q is at infinity"""
    if name.startswith("tau_"):
        return (a + TAUS[name[4:]] * b) % R_MOD == 0
    return {"inf_g2[0]": b == 0, "inf_g2[1]": a == 0, "inf_both": True}[name]


@pytest.fixture(scope="module")
def closed_pairs():
    """name -> (A [N, 8], B [N, 8], expected): B = b G and A = -(tau b) G, every third off by one; then (O, O), (O, B), (A, O)"""
    out = {}
    for name in sorted(G2_PAIRS):
        rng = random.Random("pairs " + name)
        tau = TAUS[name[4:]] if name.startswith("tau_") else 42
        logs = []
        for i in range(N_PAIRS - 3):
            b = rng.randrange(1, R_MOD)
            logs.append(((-(tau * b) - (1 if i % 3 == 2 else 0)) % R_MOD, b))
        logs += [(0, 0), (0, logs[0][1]), (logs[0][0], 0)]
        A = np.array([fp.g1_of(a) for a, _ in logs]); B = np.array([fp.g1_of(b) for _, b in logs])
        out[name] = (A, B, [VALID if _closed_form(name, a, b) else INVALID for a, b in logs])
    return out


def _pairing_many(ctx, A, B, g2):
    import torch
    n = A.shape[0]
    dA = torch.from_numpy(A.astype(np.int64)).cuda(); dB = torch.from_numpy(B.astype(np.int64)).cuda()
    out = torch.full((n + 16,), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.pairing_check_many_dev(dA.data_ptr(), dB.data_ptr(), n, g2, out.data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == 77).all()
    return got[:n].tolist()


@pytest.mark.parametrize("name", sorted(G2_PAIRS))
def test_pairing_check_many_dev_on_other_g2_pairs(ctx, closed_pairs, name):
    A, B, want = closed_pairs[name]
    if name.startswith("tau_"):
        assert want[:3] == [1, 1, 0] and want[-3:] == [1, 0, 0] and want.count(VALID) == 46
    assert _pairing_many(ctx, A, B, _g2_bytes(name)) == want


def test_cached_table_is_replaced_when_the_g2_bytes_change(ctx, closed_pairs):
    """three consecutive calls on one context with the pairs X, Y, X and the same G1 data: each answers for its own pair"""
    A, B, want_x = closed_pairs["tau_small"]
    x, y = _g2_bytes("tau_small"), _g2_bytes("tau_r_minus_1")
    assert x[:128] == y[:128] and x != y
    # under Y = {G2, -G2} the check is a == b
    want_y = [VALID if ((A[i] == B[i]).all()) else INVALID for i in range(A.shape[0])]
    assert want_y.count(VALID) == 1 and want_x != want_y
    assert _pairing_many(ctx, A, B, x) == want_x
    assert _pairing_many(ctx, A, B, y) == want_y
    assert _pairing_many(ctx, A, B, x) == want_x
    assert _pairing_many(ctx, A, B, y) == want_y
    assert _pairing_many(ctx, A, B, y) == want_y                      # and the unchanged pair keeps its table


# ---------------------------------------------------------------------------------------------- more than one chunk
def test_more_than_one_chunk_of_proofs(ctx):
    """2^16 + 5 proofs in one call: the second pass through the staging arena, the `base` offset and the packing of the survivors across
    the boundary.  VM_CHUNK is a constant, so the call cannot be smaller; the list repeats a handful of distinct proofs (verdicts are
    computed once per distinct proof), with invalid, malformed and early-rejected ones at 0, 65534 .. 65540 and the last index."""
    import plonkit_amd as pa
    rng = random.Random(65541)
    key = [rng.randrange(R_MOD) for _ in range(11)]
    forge = lambda **more: fp.forge_record(**dict(fp.random_args(rng, 15, 1, key=key), **more))
    good = [forge() for _ in range(3)]
    plus_g, px_inf = forge(variant="plus_g"), forge(variant="px_inf")
    pg_inf = fp.forge_record(**dict(fp.no_wzw(fp.random_args(rng, 15, 1, key=key)), variant="pg_inf"))
    vk = good[0].vk
    assert all(f.vk == vk for f in good + [plus_g, px_inf, pg_inf])
    distinct = {f.proof: _verdict(f) for f in good + [plus_g, px_inf, pg_inf]}
    malformed, early = good[0].proof[:-1], _bump_t_z(good[1].proof)
    distinct[malformed], distinct[early] = MALFORMED, INVALID
    for p, w in distinct.items():                                    # the host's verdict, once per distinct proof
        try:
            assert (VALID if pa.verify(vk, p, strict_inputs=False) else INVALID) == w
        except pa.PlkError:
            assert w == MALFORMED
    count = (1 << 16) + 5
    proofs = [good[i % 3].proof for i in range(count)]
    special = {0: plus_g.proof, 65534: malformed, 65535: px_inf.proof, 65536: early, 65537: plus_g.proof, 65538: pg_inf.proof, 65539: malformed,
               65540: px_inf.proof}
    assert max(special) == count - 1
    for i, p in special.items():
        proofs[i] = p
    want = np.array([distinct[p] for p in proofs], dtype=np.uint8)
    k = pa.VerificationKey(ctx, vk, strict_inputs=False)
    t0 = time.perf_counter()
    got = k.verify_many(proofs)
    print("plk_verify_many, %d proofs: %.3f s" % (count, time.perf_counter() - t0))
    assert got.shape == want.shape and np.flatnonzero(got != want).tolist() == []
    assert got[65530:].tolist() == [1, 1, 1, 1, 2, 0, 0, 0, 0, 2, 0] and k.first_bad == 0
    # the same list with a valid proof at index 0: the first bad one is now the malformed proof just before the boundary
    got = k.verify_many([good[0].proof] + proofs[1:])
    assert got[0] == VALID and k.first_bad == 65534 and np.array_equal(got[1:], want[1:])
    k.close()
