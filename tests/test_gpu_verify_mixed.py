"""plk_vkset_create / plk_verify_mixed / _packed / _dev: proofs of several verification keys in one pass, each under the key its index names.

The expected verdict is always plk_verify_ex on the host for (key, proof) — computed once per distinct pair — plus, for the four keys of
tests/gen/mixed_keys.py, the literal identity matrix: A, F, M and T differ from one another in exactly one of the three things a lane takes
through its key index (FrontVk, a fixed point, the line table), so each lookup, taken from the wrong key, flips a verdict.
  vm_front_mixed_kernel    F against A: the front end settles a proof of the other key
  vm_mul_mixed_kernel      M against A: one commitment differs, the proof reaches the pairing and fails there
  vm_pairing_mixed_kernel  T against A (and tau = 1, tau = r - 1, a G2 point at infinity): several tables in one wave, q_inf differing from lane to lane
Every assertion is an exact equality."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import plonk_oracle as po
from tests.gen import forged_proofs as fp
from tests.gen import mixed_keys as mk

pytestmark = pytest.mark.gpu

ERR_ARG = 1
VALID, INVALID, MALFORMED = 1, 0, 2
COUNTS = (1, 63, 64, 65, 131)          # one lane, either side of a wave of the front and pairing kernels, several workgroups of each kernel
PATTERNS = ("one_key", "mod", "blocks", "shuffle")


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def pack(proofs):
    """-> (blob bytes, count + 1 offsets)"""
    off = np.zeros(len(proofs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in proofs], dtype=np.uint64)
    return b"".join(proofs), off


_HOST = {}


def host_verdict(vk, proof, strict=False):
    """plk_verify_ex: 1 / 0, or 2 where it returns PLK_ERR_ARG; once per distinct (key, proof, flag)"""
    import plonkit_amd as pa
    k = (vk, proof, strict)
    if k not in _HOST:
        try:
            _HOST[k] = VALID if pa.verify(vk, proof, strict_inputs=strict) else INVALID
        except pa.PlkError as e:
            assert e.code == ERR_ARG
            _HOST[k] = MALFORMED
    return _HOST[k]


def to_dev(blob, off, key_of):
    import torch
    d_blob = torch.from_numpy(np.frombuffer(blob if blob else b"\0", dtype=np.uint8).copy()).cuda()[:len(blob)]
    return d_blob, torch.from_numpy(np.asarray(off).astype(np.int64)).cuda(), torch.from_numpy(np.asarray(key_of, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()


def all_three(ctx, kset, proofs, key_of):
    """the three calls on one batch: they must agree with one another; -> the verdict list"""
    import torch
    host = kset.verify_many(proofs, key_of)
    fb = kset.first_bad
    blob, off = pack(proofs)
    packed = kset.verify_many_packed(blob, off, key_of)
    assert kset.first_bad == fb
    d_blob, d_off, d_key = to_dev(blob, off, key_of)
    torch.cuda.synchronize()
    dev = kset.verify_many_dev(d_blob, d_off, d_key)
    ctx.synchronize()                                                 # the call does not wait
    dev = dev.cpu().numpy()
    assert host.tolist() == packed.tolist() == dev.tolist(), [i for i in range(len(proofs)) if not host[i] == packed[i] == dev[i]]
    bad = [i for i, v in enumerate(host.tolist()) if v != VALID]
    assert fb == (bad[0] if bad else None)
    return host.tolist()


class Key:
    """vk bytes, the strict flag, and a pool of proofs made for this key: `good` (what its forger calls a proof of the key) and one plus_g forgery"""

    def __init__(self, vk, good, plus_g, strict=False):
        self.vk, self.good, self.plus_g, self.strict = vk, list(good), plus_g, strict

    def host(self, proof):
        return host_verdict(self.vk, proof, self.strict)


def _mixed_key(name):
    return Key(mk.forged(name).vk, [mk.forged(name).proof] + mk.more_proofs(name, 1, "pool"), mk.forged(name, "plus_g").proof)


def _edge_key(name, strict=False, **more):
    args = dict(fp.edge_cases()[name], **more)
    f = fp.forge_record(**args)
    return Key(f.vk, [f.proof], fp.forge_record(**dict(args, variant="plus_g")).proof, strict)


def _g2_inf_key():
    """g2[1] at infinity: the verdict is "pg is O", so an ordinary forgery is invalid and the pg_inf variant is valid"""
    g2 = fp.g2_pair(42)[:128] + fp.G2_INF
    rng = random.Random("mixed: g2 at infinity")
    key = [rng.randrange(fp.R_MOD) for _ in range(11)]
    a, b = fp.random_args(rng, 1, 1, key=key), fp.random_args(rng, 1, 1, key=key)
    ordinary = fp.forge_record(**dict(a, g2=g2))
    pg_inf = fp.forge_record(**dict(fp.no_wzw(b), variant="pg_inf", g2=g2))
    assert ordinary.vk == pg_inf.vk and fp.g2_inf_verdict(pg_inf, g2) and not fp.g2_inf_verdict(ordinary, g2)
    return Key(ordinary.vk, [pg_inf.proof, ordinary.proof], fp.forge_record(**dict(a, variant="plus_g", g2=g2)).proof)


@pytest.fixture(scope="module")
def key_sets(ctx):
    """name -> (VerificationKeySet, [Key]): three keys of one G2 pair, and seven keys of five G2 pairs — tau = 42, 5, 1, r - 1 (the negated
    generator) and one with a point at infinity"""
    import plonkit_amd as pa
    keys = {"one_table": [_mixed_key(n) for n in "AFM"],
            "many_tables": [_mixed_key(n) for n in "AFMT"] + [_edge_key("tau_1"), _edge_key("tau_r_minus_1"), _g2_inf_key()]}
    sets = {name: pa.VerificationKeySet(ctx, [k.vk for k in ks]) for name, ks in keys.items()}
    assert sets["one_table"].keys == 3 and sets["one_table"].tables == 1
    assert sets["many_tables"].keys == 7 and sets["many_tables"].tables == 5
    yield {name: (sets[name], keys[name]) for name in keys}
    for s in sets.values():
        s.close()


# ---------------------------------------------------------------------------------------------- 1. the cross matrix
def test_cross_matrix_of_the_four_keys(ctx):
    import plonkit_amd as pa
    f = [mk.forged(n) for n in mk.NAMES]
    kset = pa.VerificationKeySet(ctx, [x.vk for x in f])
    assert kset.keys == 4 and kset.tables == 2
    proofs = [f[p].proof for p in range(4) for k in range(4)]
    key_of = [k for p in range(4) for k in range(4)]
    want = [VALID if p == k else INVALID for p in range(4) for k in range(4)]
    assert [host_verdict(f[k].vk, f[p].proof) for p in range(4) for k in range(4)] == want
    assert mk.cross_matrix() == [[p == k for k in range(4)] for p in range(4)]          # and the oracle says the same of the fixtures
    a = f[0].vk                                                       # each key differs from A in one thing only
    assert sum(x != y for x, y in zip(a, f[1].vk)) == 1 and f[2].vk[-256:] == a[-256:] and f[3].vk[:-128] == a[:-128] and f[3].vk != a
    assert all_three(ctx, kset, proofs, key_of) == want
    assert kset.first_bad == 1
    # and the same pairs key-major: correctness does not depend on the order of key_of
    order = sorted(range(16), key=lambda i: (key_of[i], -i))
    assert all_three(ctx, kset, [proofs[i] for i in order], [key_of[i] for i in order]) == [want[i] for i in order]
    kset.close()


# ---------------------------------------------------------------------------------------------- 2. batch sizes and key patterns
def _key_pattern(pattern, count, K):
    if pattern == "one_key":
        return [count % K] * count
    if pattern == "mod":                                              # every wave, and every group of 8 of vm_affine_kernel, is mixed
        return [i % K for i in range(count)]
    if pattern == "blocks":
        return [(i // 64) % K for i in range(count)]
    rng = random.Random("shuffle %d" % count)
    ks = [i % K for i in range(count)]
    rng.shuffle(ks)
    return ks


def _batch(keys, key_of):
    """proof i is made for key key_of[i], except: every 11th from 3 is a proof of the NEXT key under this label, every 11th from 5 is
    truncated (11 shares no factor with the 3 or 7 keys of a set, so under key = i mod K every key meets every kind), and the middle one is a
    plus_g forgery of its key (the equation at z holds: it reaches the pairing)"""
    K, count = len(keys), len(key_of)
    proofs = []
    for i, k in enumerate(key_of):
        if count > 1 and i == count // 2:
            p = keys[k].plus_g
        elif i % 11 == 3:
            p = keys[(k + 1) % K].good[0]
        elif i % 11 == 5:
            p = keys[k].good[0][:-9]
        else:
            p = keys[k].good[(i // 11) % len(keys[k].good)]
        proofs.append(p)
    return proofs


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("which", ["one_table", "many_tables"])
def test_batch_sizes_and_key_patterns(ctx, key_sets, which, count, pattern):
    kset, keys = key_sets[which]
    key_of = _key_pattern(pattern, count, len(keys))
    proofs = _batch(keys, key_of)
    want = [keys[k].host(p) for p, k in zip(proofs, key_of)]
    if count >= 63:
        assert want.count(VALID) >= count // 3 and want.count(INVALID) >= count // 11 and want.count(MALFORMED) >= count // 11
        assert want[count // 2] == INVALID and want[0] == VALID
    got = all_three(ctx, kset, proofs, key_of)
    assert got == want, [(i, key_of[i], got[i], want[i]) for i in range(count) if got[i] != want[i]]


# ---------------------------------------------------------------------------------------------- 3. a set of one key
def test_a_set_of_one_key_answers_as_the_single_key_calls(ctx, golden_dir):
    import plonkit_amd as pa
    vk = open(os.path.join(golden_dir, "vk.bin"), "rb").read()
    proof = open(os.path.join(golden_dir, "proof.bin"), "rb").read()
    flip = lambda p, at: p[:at] + bytes([p[at] ^ 1]) + p[at + 1:]
    P = po.read_proof(proof)
    P.inputs = list(P.inputs) + [1]                                   # one input too many: well-formed, and the host front end settles it as invalid
    extra_input = po.write_proof(P)
    assert host_verdict(vk, extra_input) == INVALID and host_verdict(vk, proof[:-1]) == MALFORMED
    # both drivers' ways out beside the pass: a proof cut by one byte (malformed, compacted away) and one settled early (wrong input count)
    batch = [proof, flip(proof, len(proof) - 1), proof, flip(proof, len(proof) - 200), flip(proof, 47), proof[:-1], b"", proof + b"\0", proof, flip(proof, 7),
             extra_input, proof] * 5
    assert len(batch) < 64
    key = pa.VerificationKey(ctx, vk, strict_inputs=False)
    kset = pa.VerificationKeySet(ctx, [key])
    assert kset.keys == 1 and kset.tables == 1
    single = key.verify_many(batch)
    single_fb = key.first_bad
    single_packed = key.verify_many_packed(*pack(batch))
    assert single.tolist() == single_packed.tolist() == [host_verdict(vk, p) for p in batch]
    assert sorted(set(single.tolist())) == [0, 1, 2] and single_fb == 1
    key.close()                                                       # the set keeps what it needs
    assert all_three(ctx, kset, batch, [0] * len(batch)) == single.tolist() and kset.first_bad == single_fb
    kset.close()


# ---------------------------------------------------------------------------------------------- 4. the edges, all in one set
def test_edge_keys_together_in_one_set(ctx):
    """N = 2 without inputs, N = 2^28, 300 inputs, only points at infinity, and the zero-input key once more under the strict rule: every
    proof under every key of the set, in one batch"""
    import plonkit_amd as pa
    keys = [_edge_key("random_N2^1_0_inputs"), _edge_key("random_N2^28_1_inputs"), _edge_key("random_N2^3_300_inputs"), _edge_key("all_infinity_N2"),
            _edge_key("random_N2^1_0_inputs", strict=True)]
    loaded = [pa.VerificationKey(ctx, k.vk, strict_inputs=k.strict) for k in keys]
    kset = pa.VerificationKeySet(ctx, loaded)
    for k in loaded:
        k.close()
    assert kset.keys == 5 and kset.tables == 1
    pool = [keys[0].good[0], keys[1].good[0], keys[2].good[0], keys[3].good[0], keys[0].plus_g, keys[3].plus_g, keys[2].good[0][:-1]]
    proofs = [p for p in pool for _ in keys]
    key_of = [k for _ in pool for k in range(len(keys))]
    want = [keys[k].host(p) for p, k in zip(proofs, key_of)]
    own = {(p, k): want[p * len(keys) + k] for p in range(len(pool)) for k in range(len(keys))}
    assert [own[(j, j)] for j in range(4)] == [VALID] * 4            # each proof under its own key
    assert own[(0, 4)] == INVALID and own[(3, 4)] == INVALID         # the strict rule on the two zero-input proofs: the same bytes, another flag
    assert own[(4, 0)] == INVALID and own[(6, 2)] == MALFORMED
    got = all_three(ctx, kset, proofs, key_of)
    assert got == want, [(i, key_of[i], got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    kset.close()


# ---------------------------------------------------------------------------------------------- 5. the device call
def test_device_call_with_bad_key_indices_and_offsets(ctx, key_sets):
    """an index out of range gives that proof verdict 2 and its neighbours their own; so does a bad offset pair beside it.  Only verdicts are
    read here: that the lookup touches nothing for such an index is what tests/test_verify_mixed_host.py shows."""
    import torch
    import plonkit_amd as pa
    for which in ("one_table", "many_tables"):
        kset, keys = key_sets[which]
        K = len(keys)
        key_of = [i % K for i in range(70)]
        proofs = [keys[k].good[0] for k in key_of]
        want = [keys[k].host(p) for p, k in zip(proofs, key_of)]
        blob, off = pack(proofs)
        bad_keys = list(key_of)
        for i, k in ((0, K), (5, 2 ** 32 - 1), (63, K + 1), (64, 2 ** 31), (69, K)):
            bad_keys[i] = k
        bad_off = off.copy()
        bad_off[7] = off[8] + 5                                       # pair (7, 8) decreases; proof 6 runs on into proof 7: trailing bytes
        with pytest.raises(pa.PlkError) as e:                         # the host call looks at the indices and refuses them
            kset.verify_many_packed(blob, off, bad_keys)
        assert e.value.code == ERR_ARG
        expect = list(want)
        for i in (0, 5, 63, 64, 69, 6, 7):
            expect[i] = MALFORMED
        d_blob, d_off, d_key = to_dev(blob, bad_off, bad_keys)
        torch.cuda.synchronize()
        v = kset.verify_many_dev(d_blob, d_off, d_key)
        ctx.synchronize()
        assert v.cpu().numpy().tolist() == expect
        assert kset.verify_many_packed(blob, off, key_of).tolist() == want


def test_device_call_then_an_arena_user_on_another_stream(ctx, key_sets):
    """the pattern of tests/test_gpu_verify_front.py: plk_verify_mixed_dev returns before its kernels end; a call that writes the staging
    arena on a stream of its own follows at once; then two device calls back to back on different streams queue up"""
    import struct
    import torch
    from oracle import plonk_oracle as po
    kset, keys = key_sets["many_tables"]
    count, n = 1024, 1 << 19
    key_of = _key_pattern("shuffle", count, len(keys))
    proofs = _batch(keys, key_of)
    want = [keys[k].host(p) for p, k in zip(proofs, key_of)]
    wtns = (b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, 40) + struct.pack("<I", 32) + po.BN254_PRIME_LE
            + struct.pack("<I", n) + struct.pack("<IQ", 2, 32 * n) + b"\x01" * (32 * n))
    blob, off = pack(proofs)
    assert kset.verify_many_packed(blob, off, key_of).tolist() == want      # and the arena has grown
    d_blob, d_off, d_key = to_dev(blob, off, key_of)
    d_fr = torch.zeros((n, 4), dtype=torch.int64, device="cuda:0")
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    v = kset.verify_many_dev(d_blob, d_off, d_key, stream=a)
    assert ctx.wtns_decode(wtns, d_fr, n, stream=b) == (n, None)      # returns after ITS stream; stream a has not been waited for
    a.synchronize()
    assert v.cpu().numpy().tolist() == want
    v2 = kset.verify_many_dev(d_blob, d_off, d_key, stream=a)         # a second device call queues behind the first
    v3 = kset.verify_many_dev(d_blob[:int(off[100])], d_off[:101], d_key[:100], stream=b)
    a.synchronize(); b.synchronize()
    assert v2.cpu().numpy().tolist() == want and v3.cpu().numpy().tolist() == want[:100]


# ---------------------------------------------------------------------------------------------- 6. the chunk seam
def test_more_than_one_chunk_of_mixed_proofs(ctx, key_sets):
    """2^16 + 5 proofs with key = i mod 3: the key indices of the second pass start at 65536, where i mod 3 is 1 and not 0"""
    kset, keys = key_sets["one_table"]
    count = (1 << 16) + 5
    key_of = np.arange(count, dtype=np.uint32) % 3
    proofs = [keys[k].good[0] for k in key_of.tolist()]
    special = {0: keys[0].plus_g, 65534: keys[65534 % 3].good[0][:-1], 65535: keys[0].good[0], 65536: keys[0].good[0], 65537: keys[65537 % 3].plus_g,
               65539: keys[0].good[1], 65540: keys[2].good[0]}
    for i, p in special.items():
        proofs[i] = p
    want = np.array([keys[k].host(p) for p, k in zip(proofs, key_of.tolist())], dtype=np.uint8)
    assert want[65530:].tolist() == [1, 1, 1, 1, 2, 1, 0, 0, 1, 0, 1]          # 65535 and 65536: a proof of key 0 under key 65535 mod 3 = 0 and key 65536 mod 3 = 1
    assert (65535 % 3, 65536 % 3, 65539 % 3, 65540 % 3) == (0, 1, 1, 2)
    got = kset.verify_many_packed(*pack(proofs), key_of)
    assert got.shape == want.shape and np.flatnonzero(got != want).tolist() == []
    assert kset.first_bad == 0


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(ctx, key_sets):
    import torch
    import plonkit_amd as pa
    L = pa.lib()
    kset, keys = key_sets["one_table"]
    proofs = [keys[0].good[0], keys[1].good[0]]
    blob, off = pack(proofs)
    # an empty set, too many keys, a null key
    h = ctypes.c_void_p()
    key = pa.VerificationKey(ctx, keys[0].vk, strict_inputs=False)
    one = (ctypes.c_void_p * 1)(key._h.value)
    assert L.plk_vkset_create(ctx._h, one, ctypes.c_uint32(0), ctypes.byref(h)) == ERR_ARG and not h.value
    assert L.plk_vkset_create(ctx._h, None, ctypes.c_uint32(0), ctypes.byref(h)) == ERR_ARG
    assert L.plk_vkset_create(ctx._h, one, ctypes.c_uint32(1025), ctypes.byref(h)) == ERR_ARG
    assert L.plk_vkset_create(ctx._h, (ctypes.c_void_p * 2)(key._h.value, None), ctypes.c_uint32(2), ctypes.byref(h)) == ERR_ARG
    assert L.plk_vkset_create(ctx._h, one, ctypes.c_uint32(1), None) == ERR_ARG and L.plk_vkset_create(None, one, ctypes.c_uint32(1), ctypes.byref(h)) == ERR_ARG
    with pytest.raises(pa.PlkError) as e:
        pa.VerificationKeySet(ctx, [])
    assert e.value.code == ERR_ARG
    assert L.plk_vkset_keys(None) == 0 and L.plk_vkset_tables(None) == 0
    # a freed plk_vk after plk_vkset_create is harmless
    mine = pa.VerificationKeySet(ctx, [key, key])
    key.close()
    assert mine.keys == 2 and mine.tables == 1
    assert mine.verify_many([proofs[0]] * 3, [0, 1, 0]).tolist() == [1, 1, 1] and mine.first_bad is None
    mine.close()
    # an index >= n_keys on the host calls: PLK_ERR_ARG, nothing launched, the verdict bytes untouched
    torch.cuda.synchronize()
    fb = ctypes.c_uint64(5)
    verdict = np.full(2, 77, dtype=np.uint8)
    ptrs = (ctypes.c_char_p * 2)(*proofs)
    lens = (ctypes.c_uint64 * 2)(*[len(p) for p in proofs])
    for bad in ([0, 3], [2 ** 32 - 1, 0]):
        bad_keys = np.array(bad, dtype=np.uint32)
        assert L.plk_verify_mixed(ctx._h, kset._h, ptrs, lens, bad_keys.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(2), verdict.ctypes.data_as(ctypes.c_void_p),
                                  ctypes.byref(fb)) == ERR_ARG
        assert L.plk_verify_mixed_packed(ctx._h, kset._h, blob, ctypes.c_uint64(len(blob)), off.ctypes.data_as(ctypes.c_void_p), bad_keys.ctypes.data_as(ctypes.c_void_p),
                                         ctypes.c_uint64(2), verdict.ctypes.data_as(ctypes.c_void_p), ctypes.byref(fb)) == ERR_ARG
        assert verdict.tolist() == [77, 77] and "keys" in pa.last_error()
        with pytest.raises(pa.PlkError):
            kset.verify_many(proofs, bad)
    with pytest.raises(ValueError):
        kset.verify_many(proofs, [0])
    # count == 0 launches nothing and needs no arrays; null arguments
    z, o = ctypes.c_uint64(0), ctypes.c_uint64(1)
    buf = ctypes.create_string_buffer(1)
    assert L.plk_verify_mixed(ctx._h, kset._h, None, None, None, z, buf, ctypes.byref(fb)) == 0 and fb.value == 2 ** 64 - 1
    fb.value = 5
    assert L.plk_verify_mixed_packed(ctx._h, kset._h, None, z, None, None, z, buf, ctypes.byref(fb)) == 0 and fb.value == 2 ** 64 - 1
    assert L.plk_verify_mixed_dev(ctx._h, kset._h, None, z, None, None, z, None, None) == 0
    assert kset.verify_many([], []).tolist() == [] and kset.first_bad is None
    assert kset.verify_many_packed(b"", np.zeros(1, dtype=np.uint64), []).tolist() == []
    assert L.plk_verify_mixed(ctx._h, kset._h, None, None, None, o, buf, ctypes.byref(fb)) == ERR_ARG
    assert L.plk_verify_mixed(ctx._h, None, None, None, None, z, buf, ctypes.byref(fb)) == ERR_ARG
    assert L.plk_verify_mixed_packed(ctx._h, kset._h, None, z, off.ctypes.data_as(ctypes.c_void_p), None, o, buf, ctypes.byref(fb)) == ERR_ARG
    assert L.plk_verify_mixed_dev(ctx._h, kset._h, None, z, None, None, o, None, None) == ERR_ARG
    # the offset-table rules of plk_verify_many_packed
    worse = off.copy(); worse[2] = len(blob) + 1
    with pytest.raises(pa.PlkError, match="offsets"):
        kset.verify_many_packed(blob, worse, [0, 1])
    # a commitment in flight; key indices that are not 4-byte aligned
    from oracle import oracle_lib as ol
    sc = torch.from_numpy(ol.fr_vec(list(range(1, 65))).astype(np.int64)).cuda()
    d_blob, d_off, d_key = to_dev(blob, off, [0, 1])
    ctx.srs_generate(1 << 10, 0, 42)                                  # a key for the commitment
    torch.cuda.synchronize()
    ctx.msm_enqueue_dev(sc.data_ptr(), 64)
    with pytest.raises(pa.PlkError, match="in flight"):
        kset.verify_many(proofs, [0, 1])
    with pytest.raises(pa.PlkError, match="in flight"):
        kset.verify_many_packed(blob, off, [0, 1])
    with pytest.raises(pa.PlkError, match="in flight"):
        kset.verify_many_dev(d_blob, d_off, d_key)
    ctx.msm_finish()
    assert L.plk_verify_mixed_dev(ctx._h, kset._h, ctypes.c_void_p(d_blob.data_ptr()), ctypes.c_uint64(len(blob)), ctypes.c_void_p(d_off.data_ptr()),
                                  ctypes.c_void_p(d_blob.data_ptr() + 2), ctypes.c_uint64(2), ctypes.c_void_p(d_blob.data_ptr()), None) == ERR_ARG
    with pytest.raises(ValueError, match="must be tensors on cuda"):
        kset.verify_many_dev(d_blob, d_off, d_key.cpu())
    assert all_three(ctx, kset, proofs, [0, 1]) == [1, 1]
    # the slots of plk_verify_many_last_ms after the two blocking calls
    ctx.set_kernel_timing(True)
    try:
        kset.verify_many(proofs, [0, 1])
        ms = ctx.verify_many_last_ms()
        assert len(ms) == 6 and all(t >= 0 for t in ms) and ms[2] > 0 and ms[4] > 0
        kset.verify_many_packed(blob, off, [0, 1])
        ms = ctx.verify_many_last_ms()
        assert len(ms) == 6 and ms[0] > 0 and ms[2] > 0 and ms[4] > 0
    finally:
        ctx.set_kernel_timing(False)


# ---------------------------------------------------------------------------------------------- 8. the binary
def test_cli_verify_mixed(tmp_path):
    import plonkit_amd as pa
    cli = os.path.join(os.path.dirname(pa.lib_path()), "plonkit")
    a, t = mk.forged("A"), mk.forged("T")
    vka = tmp_path / "a.vk.bin"; vka.write_bytes(a.vk)
    vkt = tmp_path / "t.vk.bin"; vkt.write_bytes(t.vk)
    pa1 = tmp_path / "a1.proof.bin"; pa1.write_bytes(a.proof)
    pa2 = tmp_path / "a2.proof.bin"; pa2.write_bytes(mk.more_proofs("A", 1, "cli")[0])
    pt1 = tmp_path / "t1.proof.bin"; pt1.write_bytes(t.proof)
    cut = tmp_path / "cut.proof.bin"; cut.write_bytes(t.proof[:40])

    def run(*args):
        return subprocess.run(["timeout", "-k", "10", "120", cli, "verify-mixed"] + [str(x) for x in args], capture_output=True, text=True, timeout=150)
    for front in ((), ("--front", "host"), ("--front", "device")):
        good = run(*front, "-v", vka, pa1, pa2, "-v", vkt, pt1)
        assert good.returncode == 0, good.stderr
        assert good.stdout.splitlines() == ["%s: valid" % f for f in (pa1, pa2, pt1)]
        # the same files with the groups exchanged, a key named twice, a truncated proof
        bad = run(*front, "-v", vkt, pa1, "-v", vka, pt1, pa2, "-v", vkt, pt1, cut)
        assert bad.returncode == 144, bad.stderr
        assert bad.stdout.splitlines() == ["%s: %s" % (f, w) for f, w in zip((pa1, pt1, pa2, pt1, cut), ("invalid", "invalid", "valid", "valid", "malformed"))]
    assert run(pa1, "-v", vka, pa2).returncode == 2                   # a proof before the first -v
    assert run("-v", vka).returncode == 2 and run("--front", "gpu", "-v", vka, pa1).returncode == 2
    assert run("-v", tmp_path / "missing.vk.bin", pa1).returncode == 101
