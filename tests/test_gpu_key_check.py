"""-m gpu: structure checks of the resident key(s) (keycheck.hip): plk_srs_check — are the monomial points P_0, tau P_0, tau^2 P_0, ...
for the tau of the key file's G2 section — and plk_srs_lagrange_check — does the Lagrange-form key belong to the monomial one.
The reference has no counterpart (bellman's Crs::read checks the curve equation only), so the referees are what is pinned:
  * valid keys: the reference's own tests/golden/setup_2pow10.key with its own G2 bytes, and crs_42 (plk_srs_generate, tau = 42)
    with plk_crs42_g2_bytes;
  * refused keys: built from valid points by construction (a point repeated, negated, swapped with its neighbour, replaced by
    infinity, a key spliced from tau = 42 and tau = 43, ...), so the verdict and the LOWEST broken link are known from how the
    key was made.  Link i is the relation P_{i+1} = tau P_i.
The form built is the one-commitment form: T = sum rho^i P_i, A = T - P_0, B = rho (T - rho^(n-1) P_{n-1}), e(A, Q_0) e(-B, Q_1) = 1.
No second implementation of the check lives here; the only arithmetic of this file is the construction of a twist point outside
the order-r subgroup (an Fq2 square root) and the pairing-free proof that it is outside ([r]Q != O by double-and-add)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_lib as ol, plonk_oracle as po
from oracle.oracle_lib import Q_MOD, R_MOD

ERR_ARG, ERR_SIZE, ERR_SRS = 1, 2, 3
SEEDS = [bytes([17 * k + 1]) * 32 for k in range(8)]             # eight fixed seeds
N = 1 << 12                                                      # size of the constructed keys


@pytest.fixture(scope="module")
def ctx():
    import plonkit_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g2_42():
    import plonkit_amd as pa
    return pa.crs42_g2_bytes()


@pytest.fixture(scope="module")
def pts42(ctx):
    ctx.srs_generate(N, 0, 42)
    return ctx.srs_download(0, N)


@pytest.fixture(scope="module")
def pts43(ctx):
    ctx.srs_generate(N, 0, 43)
    return ctx.srs_download(0, N)


def _golden_raw(golden_dir):
    return open(os.path.join(golden_dir, "setup_2pow10.key"), "rb").read()


def _neg(p):
    """-P of an affine Montgomery point that is not infinity: y -> q - y (the Montgomery form of -y)"""
    out = np.array(p, dtype=np.uint64, copy=True)
    out[4:] = ol.int_to_limbs(Q_MOD - ol.limbs_to_int(p[4:]))
    return out


def _expect_refused(ctx, g2, link):
    """refused under the eight seeds, without PLK_KEY_LOCATE no index is reported; located at `link`; the same seed twice agrees"""
    for seed in SEEDS:
        assert ctx.srs_check(g2, seed=seed) == (False, None), seed[:1].hex()
    assert ctx.srs_check(g2, seed=SEEDS[0], locate=True) == (False, link)
    assert ctx.srs_check(g2, seed=SEEDS[0], locate=True) == (False, link)
    assert ctx.srs_check(g2, seed=SEEDS[5], locate=True) == (False, link)
    assert ctx.srs_check(g2, locate=True) == (False, link)                       # OS randomness


# ------------------------------------------------------------------------------------------------ valid keys
def test_golden_key_is_valid(ctx, golden_dir):
    raw = _golden_raw(golden_dir)
    n, g2 = ctx.srs_load_key(raw)
    assert n == 1024 and g2 == raw[-256:]
    for seed in SEEDS:
        assert ctx.srs_check(g2, seed=seed) == (True, None)
    assert ctx.srs_check(g2, seed=SEEDS[0], locate=True) == (True, None)
    assert ctx.srs_check(g2) == (True, None)                                     # seed = None: OS randomness
    assert ctx.srs_check(g2, locate=True) == (True, None)


@pytest.mark.parametrize("size", ["2^12", "2^16+3", "2*chunk+5", "1"])
def test_crs42_is_valid(ctx, g2_42, size):
    import plonkit_amd as pa
    chunk = int(pa.lib().plk_key_chunk_points())
    n = {"2^12": 1 << 12, "2^16+3": (1 << 16) + 3, "2*chunk+5": 2 * chunk + 5, "1": 1}[size]
    ctx.srs_generate(n, 0, 42)
    assert ctx.srs_size() == n
    assert ctx.srs_check(g2_42, seed=SEEDS[0]) == (True, None)
    assert ctx.srs_check(g2_42, seed=SEEDS[1], locate=True) == (True, None)
    assert ctx.srs_check(g2_42) == (True, None)


def test_a_slice_of_a_valid_key_is_valid(ctx, g2_42):
    """points [1000, 6000) of a key, kept by plk_srs_load_key as a rank would: the links inside the slice hold (the link into it
    from point 999 is outside what the call sees)"""
    n = (1 << 16) + 3
    ctx.srs_generate(n, 0, 42)
    raw = ctx.srs_store_key(g2_42)
    ctx.srs_load_key(raw, first=1000, count=5000)
    assert ctx.srs_size() == 5000
    assert ctx.srs_check(g2_42, seed=SEEDS[2]) == (True, None)
    assert ctx.srs_check(g2_42, seed=SEEDS[3], locate=True) == (True, None)
    ctx.srs_generate(5000, 1000, 42)                                             # the same slice, generated
    assert ctx.srs_check(g2_42, seed=SEEDS[2]) == (True, None)


# ------------------------------------------------------------------------------------------------ refused keys
def test_a_key_of_another_tau_is_refused_at_link_0(ctx, pts43, g2_42):
    ctx.srs_upload(pts43)
    _expect_refused(ctx, g2_42, 0)


def _tampered(kind, k, pts42, ctx):
    """(points, lowest broken link)"""
    pts = pts42.copy()
    if kind == "repeat":                                         # P_k := P_{k-1}
        pts[k] = pts42[k - 1]
    elif kind == "negate":                                       # P_k := -P_k
        pts[k] = _neg(pts42[k])
    elif kind == "swap":                                         # P_k <-> P_{k+1}: what a check with constant scalars misses
        pts[k], pts[k + 1] = pts42[k + 1], pts42[k]
    elif kind == "infinity":
        pts[k] = 0
    elif kind == "splice":                                       # first k points of tau = 42, the rest 43^(k+i) G: every later link is broken too
        ctx.srs_generate_fr(N - k, k, ol.fr_mont(43))
        pts[k:] = ctx.srs_download(0, N - k)
    return pts, k - 1


@pytest.mark.parametrize("where", ["1", "n/2", "n-1"])
@pytest.mark.parametrize("kind", ["repeat", "negate", "swap", "infinity", "splice"])
def test_tampered_keys_are_refused_and_located(ctx, pts42, g2_42, kind, where):
    k = {"1": 1, "n/2": N // 2, "n-1": N - 1}[where]
    if kind == "swap" and k == N - 1:
        k = N - 2                                                # the last pair
    pts, link = _tampered(kind, k, pts42, ctx)
    assert not np.array_equal(pts, pts42)
    ctx.srs_upload(pts)
    _expect_refused(ctx, g2_42, link)


def test_an_all_infinity_key_is_refused_by_the_rule_on_the_first_point(ctx, g2_42):
    """it would pass the pairing identity trivially (A = B = O)"""
    ctx.srs_upload(np.zeros((N, 8), dtype=np.uint64))
    for seed in SEEDS:
        assert ctx.srs_check(g2_42, seed=seed) == (False, 0)
    assert ctx.srs_check(g2_42, seed=SEEDS[0], locate=True) == (False, 0)
    ctx.srs_upload(np.zeros((1, 8), dtype=np.uint64))            # n = 1
    assert ctx.srs_check(g2_42, seed=SEEDS[0]) == (False, 0)


# ------------------------------------------------------------------------------------------------ G2
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q_MOD, (a[0] * b[1] + a[1] * b[0]) % Q_MOD)


def _f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q_MOD)
    return (a[0] * n % Q_MOD, -a[1] * n % Q_MOD)


def _f2sub(a, b):
    return ((a[0] - b[0]) % Q_MOD, (a[1] - b[1]) % Q_MOD)


def _fq_sqrt(a):
    s = pow(a, (Q_MOD + 1) // 4, Q_MOD)                          # q = 3 mod 4
    return s if s * s % Q_MOD == a % Q_MOD else None


def _f2sqrt(a):
    """a square root in Fq2 = Fq[i] / (i^2 + 1), or None: (x0 + x1 i)^2 = a with x0^2 = (a0 +- |a|) / 2, x1 = a1 / (2 x0)"""
    a0, a1 = a
    if a1 == 0:
        s = _fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = _fq_sqrt(-a0 % Q_MOD)
        return None if s is None else (0, s)
    norm = _fq_sqrt((a0 * a0 + a1 * a1) % Q_MOD)
    if norm is None:
        return None
    half = pow(2, -1, Q_MOD)
    for t in ((a0 + norm) * half % Q_MOD, (a0 - norm) * half % Q_MOD):
        x0 = _fq_sqrt(t)
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, Q_MOD) % Q_MOD)
            if _f2mul(x, x) == (a0 % Q_MOD, a1 % Q_MOD):
                return x
    return None


TWIST_B = _f2mul((3, 0), _f2inv((9, 1)))                         # y^2 = x^3 + 3 / (9 + i)


def _g2_add(p, q):
    """affine addition on the twist; None is infinity"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == (0, 0):
            return None
        m = _f2mul(_f2mul((3, 0), _f2mul(p[0], p[0])), _f2inv(_f2mul((2, 0), p[1])))
    else:
        m = _f2mul(_f2sub(q[1], p[1]), _f2inv(_f2sub(q[0], p[0])))
    x = _f2sub(_f2sub(_f2mul(m, m), p[0]), q[0])
    return (x, _f2sub(_f2mul(m, _f2sub(p[0], x)), p[1]))


def _g2_mul(p, k):
    acc = None
    for bit in bin(k)[2:]:
        acc = _g2_add(acc, acc)
        if bit == "1":
            acc = _g2_add(acc, p)
    return acc


def _g2_decode(b):
    c = [int.from_bytes(b[32 * j: 32 * j + 32], "big") for j in range(4)]
    return ((c[1], c[0]), (c[3], c[2]))                          # x.c1 | x.c0 | y.c1 | y.c0


def _g2_encode(p):
    return b"".join(v.to_bytes(32, "big") for v in (p[0][1], p[0][0], p[1][1], p[1][0]))


def _twist_point_outside_the_subgroup():
    for k in range(1, 200):
        x = (k, 0)
        y = _f2sqrt(tuple((u + v) % Q_MOD for u, v in zip(_f2mul(_f2mul(x, x), x), TWIST_B)))
        if y is not None:
            q = (x, y)
            if _g2_mul(q, R_MOD) is not None:                    # (a random twist point is in the subgroup with probability ~2^-254)
                return q
    raise AssertionError("no twist point found")


def test_g2_sections_that_are_wrong(ctx, pts42, g2_42):
    import plonkit_amd as pa
    ctx.srs_upload(pts42)
    q0, q1 = g2_42[:128], g2_42[128:]
    assert ctx.srs_check(g2_42, seed=SEEDS[0]) == (True, None)
    # {Q_1, Q_0}
    for seed in SEEDS:
        assert ctx.srs_check(q1 + q0, seed=seed)[0] is False
    # a member at infinity
    inf = b"\x40" + b"\x00" * 127
    assert ctx.srs_check(q0 + inf, seed=SEEDS[0]) == (False, None)
    assert ctx.srs_check(q0 + inf, seed=SEEDS[0], locate=True) == (False, None)
    assert ctx.srs_check(inf + q1, seed=SEEDS[0]) == (False, None)
    # one byte flipped: off the twist, an argument error in plk_pairing_check's words
    for pos in (127, 255, 40):
        bad = bytearray(g2_42)
        bad[pos] ^= 1
        with pytest.raises(pa.PlkError) as e:
            ctx.srs_check(bytes(bad), seed=SEEDS[0])
        assert e.value.code == ERR_ARG and "G2 point not on the twist" in str(e.value)
    # on the twist, outside the order-r subgroup.  The arithmetic of this file is checked on the generator first: [r]Q_0 = O
    g = _g2_decode(q0)
    assert _g2_encode(g) == q0
    gy2 = _f2mul(g[1], g[1])
    assert gy2 == tuple((u + v) % Q_MOD for u, v in zip(_f2mul(_f2mul(g[0], g[0]), g[0]), TWIST_B))
    assert _g2_mul(g, R_MOD) is None and _g2_mul(g, R_MOD - 1) is not None
    assert _g2_encode(_g2_mul(g, 42)) == q1
    stray = _twist_point_outside_the_subgroup()
    assert _g2_mul(stray, R_MOD) is not None                     # [r]Q != O: pairing-free
    sb = _g2_encode(stray)
    for pair in (sb + q1, q0 + sb, sb + sb):
        for seed in SEEDS[:3]:
            assert ctx.srs_check(pair, seed=seed) == (False, None)
    assert ctx.srs_check(sb + q1, seed=SEEDS[0], locate=True) == (False, None)


# ------------------------------------------------------------------------------------------------ arguments
def test_status_codes(g2_42, pts42):
    import plonkit_amd as pa
    L = pa.lib()
    c = pa.Context(0)
    try:
        with pytest.raises(pa.PlkError) as e:
            c.srs_check(g2_42, seed=SEEDS[0])
        assert e.value.code == ERR_SRS
        with pytest.raises(pa.PlkError) as e:
            c.srs_lagrange_check(seed=SEEDS[0])
        assert e.value.code == ERR_SRS
        c.srs_upload(pts42)
        valid, bad = ctypes.c_int32(7), ctypes.c_uint64(7)
        for flags in (1, 4, 3, 0x80000000):                      # PLK_KEY_LAGRANGE is not a flag of this call
            assert L.plk_srs_check(c._h, g2_42, SEEDS[0], ctypes.c_uint32(flags), ctypes.byref(valid), ctypes.byref(bad)) == ERR_ARG
        assert L.plk_srs_check(None, g2_42, SEEDS[0], ctypes.c_uint32(0), ctypes.byref(valid), ctypes.byref(bad)) == ERR_ARG
        assert L.plk_srs_check(c._h, None, SEEDS[0], ctypes.c_uint32(0), ctypes.byref(valid), ctypes.byref(bad)) == ERR_ARG
        assert L.plk_srs_check(c._h, g2_42, SEEDS[0], ctypes.c_uint32(0), None, ctypes.byref(bad)) == ERR_ARG
        assert L.plk_srs_lagrange_check(None, SEEDS[0], ctypes.byref(valid)) == ERR_ARG
        assert L.plk_srs_lagrange_check(c._h, SEEDS[0], None) == ERR_ARG
        assert L.plk_srs_check(c._h, g2_42, SEEDS[0], ctypes.c_uint32(2), ctypes.byref(valid), None) == 0 and valid.value == 1   # bad_out may be NULL
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ no side effects
def test_the_check_only_reads(ctx, golden_dir, g2_42):
    import plonkit_amd as pa
    raw = _golden_raw(golden_dir)
    _, g2 = ctx.srs_load_key(raw)
    ctx.srs_lagrange_from_powers(10)
    rng = np.random.default_rng(11)
    vec = ol.fr_vec([int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(1024)])
    before, lag_before, commit_before = ctx.srs_download(0, 1024), ctx.srs_store_key(g2, lagrange=True), ctx.msm(vec)
    assert ctx.srs_check(g2, seed=SEEDS[0], locate=True) == (True, None)
    assert ctx.srs_check(g2_42[128:] + g2_42[:128], seed=SEEDS[0], locate=True)[0] is False
    assert ctx.srs_lagrange_check(seed=SEEDS[0]) is True
    assert np.array_equal(ctx.srs_download(0, 1024), before)
    assert ctx.srs_store_key(g2, lagrange=True) == lag_before and ctx.srs_lagrange_size() == 1024
    assert ctx.srs_store_key(g2) == raw
    assert np.array_equal(ctx.msm(vec), commit_before)
    # a borrower may run both checks; the loan stands afterwards: the lender still refuses to replace its key
    other = pa.Context(0)
    try:
        other.share_srs_from(ctx)
        assert other.srs_check(g2, seed=SEEDS[1], locate=True) == (True, None)
        assert other.srs_lagrange_check(seed=SEEDS[1]) is True
        assert np.array_equal(other.msm(vec), commit_before)
        with pytest.raises(pa.PlkError) as e:
            ctx.srs_generate(1024, 0, 42)
        assert e.value.code == ERR_ARG
        with pytest.raises(pa.PlkError) as e:
            ctx.srs_lagrange_clear()
        assert e.value.code == ERR_ARG
        assert ctx.srs_check(g2, seed=SEEDS[2]) == (True, None)                  # and the lender checks beside its borrower
    finally:
        other.close()
    ctx.srs_generate(1024, 0, 42)                                                # the loan is back
    ctx.srs_lagrange_clear()


def test_a_device_key_that_the_caller_owns(ctx, pts42, g2_42):
    """plk_srs_set_dev: borrowed memory, read only"""
    import torch
    t = torch.from_numpy(pts42.view(np.int64)).to("cuda:0")
    ctx.srs_set_dev(t, N)
    assert ctx.srs_check(g2_42, seed=SEEDS[0]) == (True, None)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint64), pts42)
    ctx.srs_upload(pts42[:16])
    del t


# ------------------------------------------------------------------------------------------------ Lagrange form
def _lagrange_points(ctx, g2):
    return po.read_crs(ctx.srs_store_key(g2, lagrange=True)).g1


def test_lagrange_keys(ctx, golden_dir, g2_42):
    import plonkit_amd as pa
    # from_powers(10) of the golden key and of crs_42
    _, g2 = ctx.srs_load_key(_golden_raw(golden_dir))
    ctx.srs_lagrange_from_powers(10)
    for seed in SEEDS:
        assert ctx.srs_lagrange_check(seed=seed) is True
    assert ctx.srs_lagrange_check() is True                                      # OS randomness
    ctx.srs_generate(1 << 12, 0, 42)                                             # a longer monomial key, the same 2^10 prefix
    ctx.srs_lagrange_from_powers(10)
    assert ctx.srs_lagrange_check(seed=SEEDS[0]) is True
    good = _lagrange_points(ctx, g2_42)
    assert good.shape == (1024, 8)
    # two entries swapped; one entry negated; one at infinity
    for what in ("swap", "negate", "infinity"):
        bad = good.copy()
        if what == "swap":
            bad[[3, 700]] = good[[700, 3]]
        elif what == "negate":
            bad[511] = _neg(good[511])
        else:
            bad[1023] = 0
        ctx.srs_lagrange_upload(bad)
        for seed in SEEDS:
            assert ctx.srs_lagrange_check(seed=seed) is False, what
        assert ctx.srs_lagrange_check() is False
    # the Lagrange form of another tau
    ctx.srs_generate(1024, 0, 43)
    ctx.srs_lagrange_from_powers(10)
    assert ctx.srs_lagrange_check(seed=SEEDS[0]) is True
    other = _lagrange_points(ctx, g2_42)
    ctx.srs_generate(1024, 0, 42)
    ctx.srs_lagrange_upload(other)
    for seed in SEEDS:
        assert ctx.srs_lagrange_check(seed=seed) is False
    # another domain: the first half of the 2^10 key is not the 2^9 key
    ctx.srs_lagrange_upload(good[:512])
    assert ctx.srs_lagrange_check(seed=SEEDS[0]) is False
    ctx.srs_lagrange_from_powers(9)
    assert ctx.srs_lagrange_check(seed=SEEDS[0]) is True
    # status codes
    ctx.srs_lagrange_upload(good)
    ctx.srs_generate(512, 0, 42)                                                 # monomial key shorter than N
    with pytest.raises(pa.PlkError) as e:
        ctx.srs_lagrange_check(seed=SEEDS[0])
    assert e.value.code == ERR_SRS
    ctx.srs_generate(1024, 0, 42)
    ctx.srs_lagrange_upload(good[:1000])                                         # not a power of two
    with pytest.raises(pa.PlkError) as e:
        ctx.srs_lagrange_check(seed=SEEDS[0])
    assert e.value.code == ERR_SIZE
    ctx.srs_lagrange_upload(good)
    assert ctx.srs_lagrange_check(seed=SEEDS[0]) is True
    ctx.set_commit_shard(512, lambda sums: None)                                 # a rank's slice: first index 512
    try:
        with pytest.raises(pa.PlkError) as e:
            ctx.srs_lagrange_check(seed=SEEDS[0])
        assert e.value.code == ERR_ARG
    finally:
        ctx.set_commit_shard(0, None)
    assert ctx.srs_lagrange_check(seed=SEEDS[0]) is True
    ctx.srs_lagrange_clear()                                                     # no Lagrange-form key
    with pytest.raises(pa.PlkError) as e:
        ctx.srs_lagrange_check(seed=SEEDS[0])
    assert e.value.code == ERR_SRS


# ------------------------------------------------------------------------------------------------ the binary
def test_binary_check_key(ctx, golden_dir, g2_42, tmp_path):
    import plonkit_amd as pa
    cli = os.path.join(os.path.dirname(pa.lib_path()), "plonkit")
    golden = os.path.join(golden_dir, "setup_2pow10.key")

    def run(*args):
        r = subprocess.run([cli, "check-key"] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        print(r.returncode, r.stdout, r.stderr)
        return r

    r = run("-m", golden)
    assert r.returncode == 0 and r.stdout == "%s: ok\n" % golden
    r = run("-m", golden, "--locate")
    assert r.returncode == 0 and r.stdout == "%s: ok\n" % golden
    # two neighbours swapped: every point is still on the curve, the key loads, link 499 is the first that fails
    raw = bytearray(_golden_raw(golden_dir))
    a, b = 8 + 64 * 500, 8 + 64 * 501
    raw[a:a + 64], raw[b:b + 64] = raw[b:b + 64], raw[a:a + 64]
    bad = tmp_path / "swapped.key"
    bad.write_bytes(bytes(raw))
    r = run("-m", bad, "--locate")
    assert r.returncode == 2 and r.stdout == "%s: INVALID, first broken link at index 499\n" % bad
    r = run("--locate", "-m", bad)
    assert r.returncode == 2 and "first broken link at index 499" in r.stdout
    r = run("-m", bad)
    assert r.returncode == 2 and r.stdout == "%s: INVALID\n" % bad
    # -l: a dump-lagrange output of the same key, and one of another tau
    circ = os.path.join(golden_dir, "circuit.r1cs.json")
    lag = tmp_path / "lag.key"
    d = subprocess.run([cli, "dump-lagrange", "-m", golden, "-c", circ, "-l", str(lag)], capture_output=True, text=True, timeout=300)
    assert d.returncode == 0, d.stderr
    r = run("-m", golden, "-l", lag)
    assert r.returncode == 0 and r.stdout == "%s: ok\n%s: ok\n" % (golden, lag)
    ctx.srs_generate(1024, 0, 43)
    key43 = tmp_path / "tau43.key"
    key43.write_bytes(ctx.srs_store_key(g2_42))
    lag43 = tmp_path / "lag43.key"
    d = subprocess.run([cli, "dump-lagrange", "-m", str(key43), "-c", circ, "-l", str(lag43)], capture_output=True, text=True, timeout=300)
    assert d.returncode == 0, d.stderr
    r = run("-m", golden, "-l", lag43)
    assert r.returncode == 2 and r.stdout == "%s: ok\n%s: INVALID\n" % (golden, lag43)
    r = run("-m", key43, "-l", lag43, "--locate")                                # tau = 43 against 42's G2 section; its own Lagrange form
    assert r.returncode == 2 and r.stdout == "%s: INVALID, first broken link at index 0\n%s: ok\n" % (key43, lag43)
    # unreadable and malformed files: 101, as the other sub-commands
    r = run("-m", tmp_path / "missing.key")
    assert r.returncode == 101
    r = run("-m", golden, "-l", tmp_path / "missing.key")
    assert r.returncode == 101
    short = tmp_path / "short.key"
    short.write_bytes(bytes(_golden_raw(golden_dir)[:5000]))
    r = run("-m", short)
    assert r.returncode == 101
