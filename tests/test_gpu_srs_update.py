"""-m gpu: contributing a secret to a resident key (srs_update.hip): plk_srs_update multiplies point i by s^(first + i) in a kernel,
plk_srs_update_verify checks the receipt.  The reference has no counterpart; the referee is the trapdoor.  crs_42 is the key of
tau = 42, so its update by s must be, byte for byte, the key of tau = 42 s that plk_srs_generate_fr computes by a different route
(a plain double-and-add of the generator per point), and g2_new must be {G2, 42 s G2} from the twist arithmetic of
tests/gen/forged_proofs.py.  Small keys and keys that are no power series also go against the oracle's G1 arithmetic.
Sizes: the smallest that cross each seam — the normalisation group of 8, the workgroup of 256, more workgroups than one, and
one pass more than the XYZZ scratch holds (CHUNK)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol
from oracle.oracle_lib import Q_MOD, R_MOD
from tests.gen import forged_proofs as fp

ERR_ARG, ERR_SIZE = 1, 2
TAU = 42
CHUNK = 1 << 22                                                  # SRS_CHUNK of csrc/srs.h: points per pass through the scratch
LAMBDA = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23      # glv_dev.h: k = 0 + 1 * lambda
S_A = 0x2b6f1d3c5a79880716253443526170fedcba98765432100123456789abcdef01 % R_MOD
S_B = 0x3041a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f % R_MOD
SCALARS = {"1": 1, "r-1": R_MOD - 1, "lambda": LAMBDA, "2": 2, "a": S_A, "b": S_B}
SEEDS = [bytes([17 * k + 1]) * 32 for k in range(8)]


@pytest.fixture(scope="module")
def pa():
    import plonkit_amd
    return plonkit_amd


@pytest.fixture(scope="module")
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(pa):
    """a second context: the keys the trapdoor predicts (plk_srs_generate_fr) are made here, the context under test is left alone"""
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g2_42(pa):
    g2 = pa.crs42_g2_bytes()
    assert g2 == fp.g2_pair(TAU)
    return g2


_G2_CACHE = {}


def _g2_pair(tau):
    tau %= R_MOD
    if tau not in _G2_CACHE:
        _G2_CACHE[tau] = fp.g2_pair(tau)
    return _G2_CACHE[tau]


def _key_of(ref, n, first, tau):
    ref.srs_generate_fr(n, first, ol.fr_mont(tau))
    return ref.srs_download(0, n)


def _neg_rows(pts, rows):
    out = pts.copy()
    for i in rows:
        if np.any(pts[i]):
            out[i, 4:] = ol.int_to_limbs(Q_MOD - ol.limbs_to_int(pts[i, 4:]))
    return out


def _rand_fr(seed, n):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(n)]


# ------------------------------------------------------------------------------------------------ the trapdoor
def test_the_scalars_are_what_they_say():
    assert S_A.bit_length() == 254 and S_B.bit_length() == 254 and pow(LAMBDA, 3, R_MOD) == 1 and LAMBDA != 1


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 255, 256, 257, 2049])
def test_update_of_crs42_is_the_key_of_42s(ctx, ref, g2_42, n):
    ctx.srs_generate(n, 0, TAU)
    old = ctx.srs_download(0, n)
    for name, s in SCALARS.items():
        ctx.srs_upload(old)
        g2_new, receipt = ctx.srs_update(g2_42, ol.fr_mont(s))
        got = ctx.srs_download(0, n)
        assert ctx.srs_size() == n
        assert np.array_equal(got, _key_of(ref, n, 0, TAU * s)), (n, name)
        assert g2_new == _g2_pair(TAU * s), name
        assert len(receipt) == 192 and receipt[64:] == _g2_pair(s)[128:], name
        if s == 1:
            assert np.array_equal(got, old)
        if s == R_MOD - 1:                                       # P'_i = (-1)^i P_i
            assert np.array_equal(got, _neg_rows(old, range(1, n, 2)))
        if n <= 64:
            for i in range(n):
                assert np.array_equal(got[i], ol.g1_mul(old[i], pow(s, i, R_MOD))), (n, name, i)


def test_one_pass_more_than_the_scratch_holds(ctx, ref, g2_42):
    n = CHUNK + 5
    ctx.srs_generate(n, 0, TAU)
    g2_new, _ = ctx.srs_update(g2_42, ol.fr_mont(S_A))
    assert g2_new == _g2_pair(TAU * S_A)
    want = _key_of(ref, n, 0, TAU * S_A)
    assert np.array_equal(ctx.srs_download(0, n), want)
    del want
    ctx.srs_generate(1, 0, TAU)                                  # (give the memory back)
    ref.srs_generate(1, 0, TAU)


def test_a_key_that_is_no_power_series(ctx, g2_42):
    """300 oracle multiples of G, infinity first, at both ends of a normalisation group, at the start of the next and last"""
    n, holes = 300, (0, 8, 15, 16, 299)
    g = ol.g1_generator()
    pts = np.stack([ol.g1_mul(g, k) for k in _rand_fr(5, n)])
    for h in holes:
        pts[h] = 0
    ctx.srs_upload(pts)
    ctx.srs_update(g2_42, ol.fr_mont(S_B))
    got = ctx.srs_download(0, n)
    for i in range(n):
        want = np.zeros(8, dtype=np.uint64) if i in holes else ol.g1_mul(pts[i], pow(S_B, i, R_MOD))
        assert np.array_equal(got[i], want), i


def test_a_slice_is_the_same_range_of_the_whole(ctx, g2_42):
    n, count = 4500, 300
    ctx.srs_generate(n, 0, TAU)
    ctx.srs_update(g2_42, ol.fr_mont(S_A))
    whole = ctx.srs_download(0, n)
    for first in (1, 255, 4097):
        ctx.srs_generate(count, first, TAU)
        g2_new, _ = ctx.srs_update(g2_42, ol.fr_mont(S_A), first=first)
        assert np.array_equal(ctx.srs_download(0, count), whole[first:first + count]), first
        assert g2_new == _g2_pair(TAU * S_A)


def test_the_index_bound(pa, ctx, ref, g2_42):
    """the table of powers reaches 2^28 - 1: refused before anything else, so no 2^28-point key is needed; the last index itself works"""
    ctx.srs_generate(4, 0, TAU)
    before = ctx.srs_download(0, 4)
    for first in ((1 << 28) - 3, 1 << 28, (1 << 64) - 2):
        with pytest.raises(pa.PlkError) as e:
            ctx.srs_update(g2_42, ol.fr_mont(2), first=first)
        assert e.value.code == ERR_SIZE and "plk_srs_update:" in str(e.value)
        with pytest.raises(pa.PlkError) as e:                    # ... before s and the G2 section are looked at
            ctx.srs_update(g2_42[128:] + b"\x00" * 128, np.zeros(4, dtype=np.uint64), first=first)
        assert e.value.code == ERR_SIZE
    assert np.array_equal(ctx.srs_download(0, 4), before)
    first = (1 << 28) - 4
    ctx.srs_generate(4, first, TAU)
    ctx.srs_update(g2_42, ol.fr_mont(S_B), first=first)
    assert np.array_equal(ctx.srs_download(0, 4), _key_of(ref, 4, first, TAU * S_B))


# ------------------------------------------------------------------------------------------------ the context afterwards
def _state(ctx, g2, vec):
    return (ctx.srs_download(0, ctx.srs_size()).tobytes(), ctx.srs_size(), ctx.srs_lagrange_size(),
            ctx.srs_store_key(g2, lagrange=True) if ctx.srs_lagrange_size() else None, ctx.msm(vec).tobytes())


def test_state_after_an_update_and_after_refused_ones(pa, ctx, g2_42):
    n = 1024
    vec = ol.fr_vec(_rand_fr(11, 1000))
    ctx.srs_generate(n, 0, TAU)
    ctx.srs_lagrange_from_powers(10)
    before = _state(ctx, g2_42, vec)                             # (the commitment builds the fixed-base table of the OLD key)
    assert before[2] == n
    # refused: s = 0, s not a residue, a G2 section off the twist or with infinity, a lent key
    flipped = bytearray(g2_42)
    flipped[200] ^= 1
    for s, g2 in ((np.zeros(4, dtype=np.uint64), g2_42), (ol.int_to_limbs(R_MOD), g2_42), (ol.fr_mont(2), bytes(flipped)),
                  (ol.fr_mont(2), g2_42[:128] + fp.G2_INF)):
        with pytest.raises(pa.PlkError) as e:
            ctx.srs_update(g2, s)
        assert e.value.code == ERR_ARG and "plk_srs_update:" in str(e.value)
        assert _state(ctx, g2_42, vec) == before
    other = pa.Context(0)
    try:
        other.share_srs_from(ctx)
        with pytest.raises(pa.PlkError) as e:
            ctx.srs_update(g2_42, ol.fr_mont(2))
        assert e.value.code == ERR_ARG and "shared with another context" in str(e.value)
        assert _state(ctx, g2_42, vec) == before
        assert other.msm(vec).tobytes() == before[4]
        # the borrower may contribute: it reads the lender's key and gets one of its own; the lender keeps its key and its Lagrange slot
        g2_b, _ = other.srs_update(g2_42, ol.fr_mont(S_A))
        assert other.srs_check(g2_b, seed=SEEDS[0]) == (True, None) and other.srs_lagrange_size() == 0
        assert _state(ctx, g2_42, vec) == before
    finally:
        other.close()
    # the update itself
    old = np.frombuffer(before[0], dtype=np.uint64).reshape(n, 8)
    g2_new, _ = ctx.srs_update(g2_42, ol.fr_mont(S_B))
    new = ctx.srs_download(0, n)
    assert ctx.srs_size() == n and ctx.srs_lagrange_size() == 0
    assert np.array_equal(new[5], ol.g1_mul(old[5], pow(S_B, 5, R_MOD)))
    assert np.array_equal(ctx.msm(vec), ol.msm(new, vec))        # a stale table would commit against the old points
    assert ctx.srs_check(g2_new, seed=SEEDS[0]) == (True, None)
    assert ctx.srs_check(g2_42, seed=SEEDS[0])[0] is False
    with pytest.raises(pa.PlkError):
        ctx.srs_lagrange_check(seed=SEEDS[0])                    # no Lagrange-form key resident


def test_a_device_key_that_the_caller_owns_is_never_written(ctx, ref, g2_42):
    import torch
    n = 777
    ctx.srs_generate(n, 0, TAU)
    old = ctx.srs_download(0, n)
    t = torch.from_numpy(old.view(np.int64)).to("cuda:0")
    ctx.srs_set_dev(t, n)
    ctx.srs_update(g2_42, ol.fr_mont(S_A))
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint64), old)
    want = _key_of(ref, n, 0, TAU * S_A)
    assert np.array_equal(ctx.srs_download(0, n), want)
    t.zero_()                                                    # the context owns its key now: the caller's memory is no part of it
    torch.cuda.synchronize()
    del t
    assert np.array_equal(ctx.srs_download(0, n), want)


# ------------------------------------------------------------------------------------------------ verification
def _updated(ctx, load, s):
    g2 = load()
    n = ctx.srs_size()
    old_p01 = ctx.srs_download(0, min(2, n))
    g2_new, receipt = ctx.srs_update(g2, ol.fr_mont(s) if s is not None else None)
    return old_p01, g2, g2_new, receipt


@pytest.mark.parametrize("which", ["golden", "crs42:1", "crs42:2", "crs42:4096"])
def test_an_honest_update_is_accepted(ctx, g2_42, golden_dir, which):
    def load():
        if which == "golden":
            return ctx.srs_load_key(open(os.path.join(golden_dir, "setup_2pow10.key"), "rb").read())[1]
        ctx.srs_generate(int(which.split(":")[1]), 0, TAU)
        return g2_42
    old_p01, g2, g2_new, receipt = _updated(ctx, load, S_A)
    before = ctx.srs_download(0, ctx.srs_size())
    for seed in SEEDS + [None]:                                  # None: OS randomness
        assert ctx.srs_update_verify(old_p01, g2, g2_new, receipt, seed=seed) == (True, "ok"), seed
    assert np.array_equal(ctx.srs_download(0, ctx.srs_size()), before)          # the call only reads
    assert ctx.srs_check(g2_new, seed=SEEDS[0]) == (True, None)


def test_dishonest_updates_are_refused(pa, ctx, g2_42):
    n = 4096
    old_p01, g2, g2_new, receipt = _updated(ctx, lambda: (ctx.srs_generate(n, 0, TAU), g2_42)[1], S_A)
    new = ctx.srs_download(0, n)
    assert ctx.srs_update_verify(old_p01, g2, g2_new, receipt, seed=SEEDS[0]) == (True, "ok")
    # point 1 of another secret
    bad = new.copy()
    bad[1] = ol.g1_mul(old_p01[1], S_A + 1)
    ctx.srs_upload(bad)
    for seed in SEEDS[:2] + [None]:
        assert ctx.srs_update_verify(old_p01, g2, g2_new, receipt, seed=seed) == (False, "p1_mismatch")
    # point 100 negated: every rule on the receipt holds, the key's own structure check says no
    bad = _neg_rows(new, [100])
    ctx.srs_upload(bad)
    for seed in SEEDS + [None]:
        assert ctx.srs_update_verify(old_p01, g2, g2_new, receipt, seed=seed) == (False, "key_structure")
    assert np.array_equal(ctx.srs_download(0, n), bad)
    # the receipt, then the G2 section, of another secret
    ctx.srs_upload(new)
    g2_other, receipt_other = pa.srs_update_receipt(ol.fr_mont(S_B), g2)
    assert ctx.srs_update_verify(old_p01, g2, g2_new, receipt_other, seed=SEEDS[0]) == (False, "p1_mismatch")
    assert ctx.srs_update_verify(old_p01, g2, g2_other, receipt, seed=SEEDS[0]) == (False, "q1_mismatch")
    assert ctx.srs_update_verify(old_p01, g2, g2, receipt, seed=SEEDS[0]) == (False, "q1_mismatch")
    assert ctx.srs_update_verify(old_p01, g2, g2_new, receipt, seed=SEEDS[0]) == (True, "ok")
    assert np.array_equal(ctx.srs_download(0, n), new)


def test_a_secret_from_the_os(ctx, g2_42):
    n = 2048
    runs = []
    for _ in range(2):
        old_p01, g2, g2_new, receipt = _updated(ctx, lambda: (ctx.srs_generate(n, 0, TAU), g2_42)[1], None)
        runs.append((ctx.srs_download(0, n), g2_new, receipt))
    (key_a, g2_a, rc_a), (key_b, g2_b, rc_b) = runs
    assert not np.array_equal(key_a, key_b) and g2_a != g2_b and rc_a != rc_b
    assert np.array_equal(key_a[0], key_b[0]) and g2_a != g2_42
    for key, g2_new, mine, theirs in ((key_a, g2_a, rc_a, rc_b), (key_b, g2_b, rc_b, rc_a)):
        ctx.srs_upload(key)
        assert ctx.srs_update_verify(old_p01, g2, g2_new, mine) == (True, "ok")
        assert ctx.srs_update_verify(old_p01, g2, g2_new, theirs)[0] is False


# ------------------------------------------------------------------------------------------------ the binary
def test_binary_contribute_and_check(pa, golden_dir, tmp_path):
    cli = os.path.join(os.path.dirname(pa.lib_path()), "plonkit")

    def f(name):
        return str(tmp_path / name)

    def run(*args):
        r = subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        print(args[0], r.returncode, r.stdout, r.stderr[-400:])
        return r

    assert run("setup", "-p", 10, "-m", f("old.key")).returncode == 0
    for k in ("a", "b"):
        assert run("contribute", "-m", f("old.key"), "-o", f(k + ".key"), "-r", f(k + ".rcpt")).returncode == 0
        assert os.path.getsize(f(k + ".rcpt")) == 192 and os.path.getsize(f(k + ".key")) == os.path.getsize(f("old.key"))
    assert open(f("a.key"), "rb").read() != open(f("b.key"), "rb").read()
    r = run("check-contribution", "-m", f("old.key"), "-n", f("a.key"), "-r", f("a.rcpt"))
    assert r.returncode == 0 and r.stdout.startswith(f("a.key") + ": ok")
    assert run("check-key", "-m", f("a.key")).returncode == 0
    for new, rcpt in (("a.key", "b.rcpt"), ("b.key", "a.rcpt")):                # the receipts swapped
        r = run("check-contribution", "-m", f("old.key"), "-n", f(new), "-r", f(rcpt))
        assert r.returncode == 2 and r.stdout.startswith(f(new) + ": INVALID, ") and r.stdout.count("\n") == 1
    # an existing output is not overwritten without --overwrite
    assert run("contribute", "-m", f("old.key"), "-o", f("a.key"), "-r", f("c.rcpt")).returncode == 101
    # a key with two neighbours swapped: every point on the curve, the key loads, and is refused before anything is multiplied
    raw = bytearray(open(f("old.key"), "rb").read())
    a, b = 8 + 64 * 500, 8 + 64 * 501
    raw[a:a + 64], raw[b:b + 64] = raw[b:b + 64], raw[a:a + 64]
    (tmp_path / "bad.key").write_bytes(bytes(raw))
    r = run("contribute", "-m", f("bad.key"), "-o", f("bad_out.key"), "-r", f("bad.rcpt"))
    assert r.returncode == 2 and not os.path.exists(f("bad_out.key")) and not os.path.exists(f("bad.rcpt"))
    # a proof from the contributed key
    circ, wit = os.path.join(golden_dir, "circuit.r1cs.json"), os.path.join(golden_dir, "witness.json")
    assert run("export-verification-key", "-m", f("a.key"), "-c", circ, "-v", f("vk.bin")).returncode == 0
    assert run("prove", "-m", f("a.key"), "-c", circ, "-w", wit, "-p", f("proof.bin"), "-j", f("p.json"), "-i", f("i.json")).returncode == 0
    assert run("verify", "-p", f("proof.bin"), "-v", f("vk.bin")).returncode == 0
    # ... which the old key's verification key refuses
    assert run("export-verification-key", "-m", f("old.key"), "-c", circ, "-v", f("vk_old.bin")).returncode == 0
    assert run("verify", "-p", f("proof.bin"), "-v", f("vk_old.bin")).returncode != 0
