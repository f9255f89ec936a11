"""plk_verify_many_packed / plk_verify_many_dev / plk_verify_front_dev on the GPU: the verifier's front end (parser, Keccak transcript, the
equation at z, the 25 flattened scalars) as a kernel over raw proof bytes, one proof per lane (verify_front.hip).  The front kernel's output
is compared word for word with plk_verify_terms, whole calls proof by proof with plk_verify_many and plk_verify_ex, forged proofs with the
forger's own assertion.  Honest proofs come from the synthetic generator as in tests/test_gpu_verify_many.py (the tampering list is copied
from there), forged ones from tests/gen/forged_proofs.py.  Host answers are computed once per distinct proof and shared."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import R_MOD
from tests.gen import forged_proofs as fp

pytestmark = pytest.mark.gpu

ERR_ARG = 1
VALID, INVALID, MALFORMED = 1, 0, 2


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


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


def pack(proofs):
    """-> (blob bytes, count + 1 offsets)"""
    off = np.zeros(len(proofs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in proofs], dtype=np.uint64)
    return b"".join(proofs), off


def host_verdict(vk, proof, strict=False):
    """plk_verify_ex: 1 / 0, or 2 where it returns PLK_ERR_ARG"""
    import plonkit_amd as pa
    try:
        return VALID if pa.verify(vk, proof, strict_inputs=strict) else INVALID
    except pa.PlkError as e:
        assert e.code == ERR_ARG
        return MALFORMED


def host_terms(vk, proof, strict=False):
    """plk_verify_terms -> (state, points [25, 8], scalars [25, 4]); zeros unless state is 1"""
    import plonkit_amd as pa
    try:
        pts, sc, early = pa.verify_terms(vk, proof, strict)
    except pa.PlkError as e:
        assert e.code == ERR_ARG
        return MALFORMED, np.zeros((25, 8), dtype=np.uint64), np.zeros((25, 4), dtype=np.uint64)
    return (1 if early else 0), pts, sc


def front_dev(ctx, key, proofs, stream=None):
    """plk_verify_front_dev over the packed proofs -> (state [n], points [n, 25, 8], scalars [n, 25, 4]); 16 guard bytes behind the states"""
    import torch
    blob, off = pack(proofs)
    n = len(proofs)
    d_blob = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_pts = torch.full((n, 25, 8), -1, dtype=torch.int64, device="cuda:0")
    d_sc = torch.full((n, 25, 4), -1, dtype=torch.int64, device="cuda:0")
    d_state = torch.full((n + 16,), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.verify_front_dev(key, d_blob, len(blob), d_off, n, d_pts, d_sc, d_state, stream)
    ctx.synchronize()
    torch.cuda.synchronize()
    state = d_state.cpu().numpy()
    assert (state[n:] == 77).all()                                    # nothing behind the last state byte is written
    return state[:n], d_pts.cpu().numpy().view(np.uint64), d_sc.cpu().numpy().view(np.uint64)


def assert_front_matches_terms(ctx, key, vk, proofs, terms=None, strict=False):
    terms = terms or [host_terms(vk, p, strict) for p in proofs]
    state, pts, sc = front_dev(ctx, key, proofs)
    assert state.tolist() == [t[0] for t in terms]
    for i, (st, hp, hs) in enumerate(terms):
        assert np.array_equal(pts[i], hp) and np.array_equal(sc[i], hs), (i, st)
    return state


# ---------------------------------------------------------------------------------------------- honest proofs of one circuit
class Batch:
    """200 proofs of one circuit, its key, a proof of another circuit, and the host's answers per proof (cached)"""

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
        other = pa.Circuit.synthetic_ex(200, 777, 1)
        s2 = pa.SetupForProver(ctx, other)
        self.foreign = s2.prove(other)
        s2.close(); other.close()
        self._host, self._terms = {}, {}

    def host(self, proof):
        if proof not in self._host:
            self._host[proof] = host_verdict(self.vk, proof)
        return self._host[proof]

    def terms(self, proof):
        if proof not in self._terms:
            self._terms[proof] = host_terms(self.vk, proof)
        return self._terms[proof]

    def mixed(self, count, seed):
        """count proofs: honest ones, every tampering, the foreign proof, and malformed proofs of ODD lengths between good ones, so that good
        proofs start at odd byte addresses of the blob"""
        rng = random.Random(seed)
        proofs = list(self.proofs[:count])
        g = self.proofs[3]
        odd = [g[:-7 if len(g) % 2 == 0 else -8], g[:17], g + b"\0" if len(g) % 2 == 0 else g + b"\0\0", b""]
        assert all(len(p) % 2 == 1 for p in odd[:3])
        bad = tamperings(g) + [self.foreign] + odd
        for i, b in zip(rng.sample(range(count), min(len(bad), count // 2)), bad):
            proofs[i] = b
        return proofs


@pytest.fixture(scope="module")
def batch(ctx):
    return Batch(ctx)


@pytest.fixture(scope="module")
def key(ctx, batch):
    import plonkit_amd as pa
    k = pa.VerificationKey(ctx, batch.vk, strict_inputs=False)
    yield k
    k.close()


# ---------------------------------------------------------------------------------------------- 1. the front kernel against the host terms
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_front_kernel_against_verify_terms(ctx, batch, key, count):
    """the wave seams; each batch (but the single proof) mixes the three states and proofs of different lengths"""
    proofs = batch.mixed(count, 500 + count)
    terms = [batch.terms(p) for p in proofs]
    states = [t[0] for t in terms]
    if count > 1:
        assert states.count(1) >= count // 2 and states.count(0) >= 5 and states.count(2) >= 3
        assert any(off % 2 == 1 and st == 1 for off, st in zip(pack(proofs)[1][:-1].tolist(), states))   # a good proof at an odd address
    assert_front_matches_terms(ctx, key, batch.vk, proofs, terms)


def test_front_kernel_on_a_torch_stream(ctx, batch, key):
    import torch
    proofs = batch.mixed(65, 77)
    s = torch.cuda.Stream()
    state, pts, sc = front_dev(ctx, key, proofs, stream=s)
    s.synchronize()
    assert state.tolist() == [batch.terms(p)[0] for p in proofs]


@pytest.mark.parametrize("num_inputs", [0, 1, 2, 40])
def test_front_kernel_and_packed_call_by_input_count(ctx, num_inputs):
    """forged proofs of keys with 0, 1, 2 and 40 public inputs: the Lagrange loop and the input absorption; valid, W_z + G (reaches the pairing,
    invalid), t(z) + 1 (settled by the equation at z) and a cut proof"""
    import plonkit_amd as pa
    rng = random.Random(900 + num_inputs)
    keyd = [rng.randrange(R_MOD) for _ in range(11)]
    fs = [fp.forge_record(**dict(fp.random_args(rng, 31, num_inputs, key=keyd), variant=v)) for v in (None, "plus_g", None)]
    vk = fs[0].vk
    P = po.read_proof(fs[2].proof)
    P.quotient_polynomial_at_z = (P.quotient_polynomial_at_z + 1) % R_MOD
    proofs = [fs[0].proof, fs[1].proof, po.write_proof(P), fs[0].proof[:-33], fs[2].proof]
    want = [VALID, INVALID, INVALID, MALFORMED, VALID]
    assert [f.valid for f in fs] == [True, False, True]
    k = pa.VerificationKey(ctx, vk, strict_inputs=False)
    try:
        state = assert_front_matches_terms(ctx, k, vk, proofs)
        assert state.tolist() == [1, 1, 0, 2, 1]
        assert k.verify_many_packed(*pack(proofs)).tolist() == want and k.first_bad == 1
    finally:
        k.close()


# ---------------------------------------------------------------------------------------------- 2. whole calls
@pytest.mark.parametrize("count", [65, 200])
def test_packed_and_dev_calls_match_verify_many_and_verify_ex(ctx, batch, key, count):
    import torch
    proofs = batch.mixed(count, 1000 + count)
    want = [batch.host(p) for p in proofs]
    assert want.count(MALFORMED) >= 3 and want.count(INVALID) >= 5 and want.count(VALID) >= count // 2
    assert key.verify_many(proofs).tolist() == want
    first = min(i for i, w in enumerate(want) if w != VALID)
    assert key.first_bad == first
    blob, off = pack(proofs)
    got = key.verify_many_packed(blob, off)
    assert got.dtype == np.uint8 and got.tolist() == want and key.first_bad == first
    d_blob = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    v = key.verify_many_dev(d_blob, d_off, stream=s)                  # a torch tensor filled on a stream that is not the default one
    assert v.dtype == torch.uint8 and v.is_cuda and v.shape == (count,)
    s.synchronize()
    assert v.cpu().numpy().tolist() == want
    v2 = key.verify_many_dev(d_blob, d_off)                           # and on the context's own stream
    ctx.synchronize()
    assert v2.cpu().numpy().tolist() == want


def test_all_valid_and_all_invalid(ctx, batch, key):
    good = batch.proofs[:70]
    assert key.verify_many_packed(*pack(good)).tolist() == [1] * 70 and key.first_bad is None
    worse = [_with(p, opening_at_z_proof=lambda c, P=po.read_proof(p): P.opening_at_z_omega_proof) for p in batch.proofs[:3]]   # these reach the pairing
    worse += [_with(p, quotient_polynomial_at_z=lambda x: (x + 1) % R_MOD) for p in batch.proofs[3:6]]
    assert [batch.host(p) for p in worse] == [INVALID] * 6
    assert key.verify_many_packed(*pack(worse)).tolist() == [0] * 6 and key.first_bad == 0
    assert key.verify_many_packed(*pack([b"", b""])).tolist() == [2, 2]            # an empty blob


def test_device_call_then_an_arena_user_on_another_stream(ctx, batch, key):
    """plk_verify_many_dev returns before its kernels end (about 90 ms of pairing here).  A call that writes the context's staging arena on a
    stream of its own choice follows at once, with no wait in between: plk_wtns_decode of 2^19 elements, 16 MB over the start of the arena.
    The verdicts must be the host's — the device call's working memory is not the arena."""
    import struct
    import torch
    count, n = 2048, 1 << 19
    proofs = [batch.proofs[i % 200] for i in range(count)]
    for i, b in zip(range(5, count, 97), tamperings(batch.proofs[3]) + [batch.proofs[7][:-5]]):
        proofs[i] = b
    want = [batch.host(p) for p in proofs]
    assert want.count(VALID) > 2000 and want.count(INVALID) >= 5 and want.count(MALFORMED) == 1
    wtns = (b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, 40) + struct.pack("<I", 32) + po.BN254_PRIME_LE
            + struct.pack("<I", n) + struct.pack("<IQ", 2, 32 * n) + b"\x01" * (32 * n))
    blob, off = pack(proofs)
    key.verify_many_packed(blob, off)                                 # the arena has grown past the first 16 MB (11 points x 64 B x 2048 = 1.4 MB of points, then scalars, products)
    d_blob = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_fr = torch.zeros((n, 4), dtype=torch.int64, device="cuda:0")
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    v = key.verify_many_dev(d_blob, d_off, stream=a)
    assert ctx.wtns_decode(wtns, d_fr, n, stream=b) == (n, None)      # returns after ITS stream; stream a has not been waited for
    a.synchronize()
    assert v.cpu().numpy().tolist() == want
    v2 = key.verify_many_dev(d_blob, d_off, stream=a)                 # two device calls back to back on different streams queue up
    v3 = key.verify_many_dev(d_blob[:int(off[100])], d_off[:101], stream=b)
    a.synchronize(); b.synchronize()
    assert v2.cpu().numpy().tolist() == want and v3.cpu().numpy().tolist() == want[:100]


def test_device_call_refuses_host_tensors(ctx, batch, key):
    import torch
    blob, off = pack(batch.proofs[:2])
    h_blob, h_off = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()), torch.from_numpy(off.astype(np.int64))
    for b, o in ((h_blob, h_off), (h_blob.cuda(), h_off), (h_blob, h_off.cuda())):
        with pytest.raises(ValueError, match="must be tensors on cuda"):
            key.verify_many_dev(b, o)
    v = key.verify_many_dev(h_blob.cuda(), h_off.cuda())
    ctx.synchronize()                                                 # the call does not wait
    assert v.cpu().numpy().tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------- 3. forged-valid families
NAMED = dict(fp.edge_cases(), **fp.broken_cases())


@pytest.mark.parametrize("name", sorted(NAMED))
def test_forged_proofs_through_the_packed_call(ctx, name):
    """infinity points, zero scalars, equal consecutive terms, N = 2 and 2^28, trapdoors 1 and r - 1: the verdict is the forger's own assertion
    (a "valid" needs every product exact), and the front kernel's terms are plk_verify_terms's"""
    import plonkit_amd as pa
    f = fp.forge_record(**NAMED[name])
    want = VALID if f.valid else INVALID
    k = pa.VerificationKey(ctx, f.vk, strict_inputs=False)
    try:
        proofs = [f.proof, f.proof[:-1], f.proof]
        assert k.verify_many_packed(*pack(proofs)).tolist() == [want, MALFORMED, want]
        assert k.first_bad == (1 if f.valid else 0)
        assert_front_matches_terms(ctx, k, f.vk, proofs)
    finally:
        k.close()


G2_WITH_INFINITY = {"g2[0]": lambda g: fp.G2_INF + g[128:], "g2[1]": lambda g: g[:128] + fp.G2_INF, "both": lambda g: fp.G2_INF * 2}


@pytest.mark.parametrize("which", sorted(G2_WITH_INFINITY))
def test_keys_with_g2_at_infinity(ctx, which):
    import plonkit_amd as pa
    g2 = G2_WITH_INFINITY[which](fp.g2_pair(42))
    rng = random.Random("g2 at infinity " + which)
    keyd = [rng.randrange(R_MOD) for _ in range(11)]
    proofs, want, vk = [], [], None
    for i in range(8):
        variant = (None, "px_inf", "pg_inf", "plus_g")[i % 4]
        args = fp.random_args(rng, 1, 1, key=keyd)
        f = fp.forge_record(**dict(fp.no_wzw(args) if variant == "pg_inf" else args, variant=variant, g2=g2))
        vk = f.vk
        proofs.append(f.proof); want.append(VALID if fp.g2_inf_verdict(f, g2) else INVALID)
    assert want == {"g2[0]": [0, 1, 0, 0] * 2, "g2[1]": [0, 0, 1, 0] * 2, "both": [1] * 8}[which]
    k = pa.VerificationKey(ctx, vk, strict_inputs=False)
    assert k.verify_many_packed(*pack(proofs)).tolist() == want
    k.close()


# ---------------------------------------------------------------------------------------------- 4. bad offset tables
def test_bad_offset_tables(ctx, batch, key):
    """the host call refuses the table; the device call gives the affected proof verdict 2 and its neighbours their own.  Only verdicts are
    read here: that the kernel reads nothing outside a proof is what the CPU sanitizer run of the same code shows."""
    import torch
    import plonkit_amd as pa
    proofs = batch.proofs[10:16]
    blob, off = pack(proofs)
    decreasing = off.copy(); decreasing[3] = off[4] + 5               # pair (3, 4) decreases; proof 2 now runs on into proof 3: trailing bytes
    past = off.copy(); past[6] = len(blob) + 10                       # the last proof reaches past the blob
    for bad in (decreasing, past):
        with pytest.raises(pa.PlkError) as e:
            key.verify_many_packed(blob, bad)
        assert e.value.code == ERR_ARG
    d_blob = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    for bad, want in ((decreasing, [1, 1, 2, 2, 1, 1]), (past, [1, 1, 1, 1, 1, 2])):
        d_off = torch.from_numpy(bad.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        v = key.verify_many_dev(d_blob, d_off)
        ctx.synchronize()
        assert v.cpu().numpy().tolist() == want
    assert key.verify_many_packed(blob, off).tolist() == [1] * 6


# ---------------------------------------------------------------------------------------------- 5. arena and refusals
def test_more_than_one_chunk_of_packed_proofs(ctx):
    """2^16 + 5 proofs in one packed call: the second pass through the arena, its offsets and its slice of the blob.  The list repeats a
    handful of distinct proofs (the host's verdict is computed once per distinct proof), with the others around the boundary."""
    import plonkit_amd as pa
    rng = random.Random(65541)
    keyd = [rng.randrange(R_MOD) for _ in range(11)]
    forge = lambda **more: fp.forge_record(**dict(fp.random_args(rng, 15, 1, key=keyd), **more))
    good = [forge() for _ in range(3)]
    plus_g, px_inf = forge(variant="plus_g"), forge(variant="px_inf")
    vk = good[0].vk
    distinct = {f.proof: (VALID if f.valid else INVALID) for f in good + [plus_g, px_inf]}
    P = po.read_proof(good[1].proof)
    P.quotient_polynomial_at_z = (P.quotient_polynomial_at_z + 1) % R_MOD
    malformed, early = good[0].proof[:-1], po.write_proof(P)
    distinct[malformed], distinct[early] = MALFORMED, INVALID
    for p, w in distinct.items():
        assert host_verdict(vk, p) == w
    count = (1 << 16) + 5
    proofs = [good[i % 3].proof for i in range(count)]
    special = {0: plus_g.proof, 65534: malformed, 65535: px_inf.proof, 65536: early, 65537: plus_g.proof, 65539: malformed, 65540: px_inf.proof}
    for i, p in special.items():
        proofs[i] = p
    want = np.array([distinct[p] for p in proofs], dtype=np.uint8)
    k = pa.VerificationKey(ctx, vk, strict_inputs=False)
    got = k.verify_many_packed(*pack(proofs))
    assert got.shape == want.shape and np.flatnonzero(got != want).tolist() == []
    assert got[65530:].tolist() == [1, 1, 1, 1, 2, 0, 0, 0, 1, 2, 0] and k.first_bad == 0
    k.close()


def test_no_allocation_once_the_arena_has_grown(ctx, batch, key):
    """the method of tests/test_gpu_verify_many.py: free device memory does not move over repeat calls.  The device call goes through the C
    ABI with a verdict tensor made beforehand, so that torch allocates nothing in between either."""
    import torch
    import plonkit_amd as pa
    blob, off = pack(batch.proofs[:120])
    small = pack(batch.proofs[:50])
    d_blob = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    v = torch.zeros(120, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()

    def dev_call():
        assert pa.lib().plk_verify_many_dev(ctx._h, key._h, ctypes.c_void_p(d_blob.data_ptr()), ctypes.c_uint64(len(blob)), ctypes.c_void_p(d_off.data_ptr()),
                                            ctypes.c_uint64(120), ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(s.cuda_stream)) == 0
        s.synchronize()
    key.verify_many_packed(blob, off)
    dev_call()                                                       # creates the two events of the stream hand-over
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    key.verify_many_packed(blob, off)
    key.verify_many_packed(*small)
    v.zero_()
    dev_call()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == before
    assert v.cpu().numpy().tolist() == [1] * 120


def test_refusals(ctx, batch, key):
    import torch
    import plonkit_amd as pa
    L = pa.lib()
    blob, off = pack(batch.proofs[:2])
    # a commitment in flight
    sc = torch.from_numpy(ol.fr_vec(list(range(1, 65))).astype(np.int64)).cuda()
    d_blob = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    ctx.msm_enqueue_dev(sc.data_ptr(), 64)
    with pytest.raises(pa.PlkError, match="in flight") as e:
        key.verify_many_packed(blob, off)
    assert e.value.code == ERR_ARG
    with pytest.raises(pa.PlkError, match="in flight"):
        key.verify_many_dev(d_blob, d_off)
    with pytest.raises(pa.PlkError, match="in flight"):
        front_dev(ctx, key, batch.proofs[:2])
    ctx.msm_finish()
    assert key.verify_many_packed(blob, off).tolist() == [1, 1]
    # count == 0 launches nothing and needs no arrays; null arguments
    fb = ctypes.c_uint64(5)
    z = ctypes.c_uint64(0)
    assert L.plk_verify_many_packed(ctx._h, key._h, None, z, None, z, ctypes.create_string_buffer(1), ctypes.byref(fb)) == 0 and fb.value == 2 ** 64 - 1
    assert key.verify_many_packed(b"", np.zeros(1, dtype=np.uint64)).tolist() == [] and key.first_bad is None
    assert L.plk_verify_many_dev(ctx._h, key._h, None, z, None, z, None, None) == 0
    assert L.plk_verify_front_dev(ctx._h, key._h, None, z, None, z, None, None, None, None) == 0
    one = ctypes.c_uint64(1)
    assert L.plk_verify_many_packed(ctx._h, key._h, None, z, None, one, ctypes.create_string_buffer(1), ctypes.byref(fb)) == ERR_ARG
    assert L.plk_verify_many_packed(ctx._h, None, None, z, None, z, ctypes.create_string_buffer(1), ctypes.byref(fb)) == ERR_ARG
    assert L.plk_verify_many_dev(ctx._h, key._h, None, z, None, one, None, None) == ERR_ARG
    assert L.plk_verify_front_dev(ctx._h, key._h, None, z, None, one, None, None, None, None) == ERR_ARG
    with pytest.raises(pa.PlkError) as e:                             # points not 16-byte aligned
        ctx.verify_front_dev(key, d_blob, len(blob), d_off, 2, d_blob.data_ptr() + 8, d_blob.data_ptr(), d_blob.data_ptr())
    assert e.value.code == ERR_ARG


def test_timing_slots_of_the_single_key_calls(ctx, batch, key):
    """the slots of plk_verify_many_last_ms after the two blocking calls, as tests/test_gpu_verify_mixed.py asks of the mixed ones: [0] is the
    host's flattening or, for the packed call, the front kernel; [2] the multiplications, [4] the pairing"""
    proofs = batch.proofs[:2]
    ctx.set_kernel_timing(True)
    try:
        assert key.verify_many(proofs).tolist() == [1, 1]
        ms = ctx.verify_many_last_ms()
        assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[2] > 0 and ms[4] > 0
        assert key.verify_many_packed(*pack(proofs)).tolist() == [1, 1]
        ms = ctx.verify_many_last_ms()
        assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[0] > 0 and ms[2] > 0 and ms[4] > 0
    finally:
        ctx.set_kernel_timing(False)


def test_one_key_from_two_contexts(ctx, batch, key):
    import plonkit_amd as pa
    other = pa.Context(0)
    proofs = batch.proofs[:9] + [batch.foreign, batch.proofs[0][:-3]]
    want = [batch.host(p) for p in proofs]
    assert key.verify_many_packed(*pack(proofs), ctx=other).tolist() == want
    assert key.verify_many_packed(*pack(proofs)).tolist() == want
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
        assert k.verify_many_packed(*pack([proof, proof])).tolist() == [int(pa.verify(vk, proof, strict_inputs=strict))] * 2 == [0 if strict else 1] * 2
        assert_front_matches_terms(ctx, k, vk, [proof, proof], strict=strict)
        k.close()


# ---------------------------------------------------------------------------------------------- 6. the binary
def test_cli_verify_many_front_device(batch, tmp_path):
    import plonkit_amd as pa
    cli = os.path.join(os.path.dirname(pa.lib_path()), "plonkit")
    vkp = tmp_path / "vk.bin"; vkp.write_bytes(batch.vk)
    files = [tmp_path / ("p%d.bin" % i) for i in range(5)]
    bent = _with(batch.proofs[1], opening_at_z_proof=lambda c: po.read_proof(batch.proofs[1]).opening_at_z_omega_proof)
    for f, p in zip(files, (batch.proofs[0], bent, batch.proofs[2], batch.proofs[3][:41], b"")):
        f.write_bytes(p)

    def run(names, *flags):
        return subprocess.run(["timeout", "-k", "10", "120", cli, "verify-many", "-v", str(vkp)] + list(flags) + [str(f) for f in names], capture_output=True, text=True, timeout=150)
    for names in (files, [files[0], files[2]]):
        host, dev = run(names), run(names, "--front", "device")
        assert dev.stdout == host.stdout and dev.returncode == host.returncode, dev.stderr
        assert run(names, "--front", "host").stdout == host.stdout
    assert host.returncode == 0 and host.stdout.count(": valid") == 2
    mixed = run(files, "--front", "device")
    assert mixed.returncode == 144
    assert mixed.stdout.splitlines() == ["%s: %s" % (f, w) for f, w in zip(files, ("valid", "invalid", "valid", "malformed", "malformed"))]
    assert run(files[:1], "--front", "gpu").returncode == 2
