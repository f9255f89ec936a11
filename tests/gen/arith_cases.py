"""Cases, the integer model and the build / run helpers for the known-answer tests of the device primitives (tests/host/arith_kat.hip).

Python owns the operands and the expected answers.  Every expected value comes from the mathematical definition the header comments give
(Python integers, `pow`, `%`), never from the 8 x 32-bit layer, the oracle library or a port of the function under test:

    mulw(a, b)        = (A*B + m*p) >> 261,  m = -A*B*p^-1 mod 2^261            (Montgomery reduction is unique)
    mul_tw3(x, W)     = (X0*W0 + X1*W1 + X2*W2 + m*p) >> 87,  m likewise mod 2^87
    subk(a, b)        = A + k*p - B        neg2(a) = 2p - A        normw / pack / unpack keep the integer
    csub_p, reduce_full, reduce_small, s_from_w: the canonical residue
    curve operations: a plain affine BN254 group law; XYZZ results are brought to affine with integers (x = X/ZZ, y = Y/ZZZ, ZZ^3 == ZZZ^2)
    g1_mul_scalar*(b, k) = k * b with that group law: every base is m * (1, 2) for a known m, so the expected point is (k m mod r) * (1, 2)

where A is the integer value of a limb vector (sum l[i] * 2^(29 i) on the lazy layer, 2^(32 i) on the packed one).  generate() builds the groups
from a fixed seed, write_cases() / read_results() speak the program's file format, check_group() compares one group and raises an AssertionError
that names the primitive and prints the operands of the first wrong case.
"""
import concurrent.futures
import itertools
import os
import random
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
MOD = (R_MOD, Q_MOD)
FIELD_NAME = ("Fr", "Fq")
M29 = (1 << 29) - 1
R256, R261 = 1 << 256, 1 << 261
MULW_A_LIMB_MAX = 3280000000            # field29_dev.h
MULTW3_X_LIMB_MAX = 3600000000
LAMBDA = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23     # glv_dev.h
CHAIN_STEPS = 32
RANDOM_CASES = 4096
KAT_PARTS = 12                          # translation units of arith_kat.hip (KAT_PART)
MAX_LOG_N = 28                          # the 2-adicity of r - 1: the largest transform
# glv_dev.h: the reduced lattice basis (A1, -B1N), (A2, B2) of {(a, b): a + b lambda = 0 mod r}
GLV_A1, GLV_B1N = 0x6f4d8248eeb859fc8211bbeb7d4f1128, 0x89d3256894d213e3
GLV_A2, GLV_B2 = 0x89d3256894d213e3, 0x6f4d8248eeb859fd0be4e1541221250b

# name: (id, in_words, out_words, fields, device_only)       (the same table as KAT_OPS in arith_kat.hip; the program refuses a group that disagrees)
OPS = {
    "F_ADD": (1, 16, 8, (0, 1), False), "F_SUB": (2, 16, 8, (0, 1), False), "F_NEG": (3, 8, 8, (0, 1), False), "F_DBL": (4, 8, 8, (0, 1), False),
    "F_MUL": (5, 16, 8, (0, 1), False), "F_SQR": (6, 8, 8, (0, 1), False), "F_INV": (7, 8, 8, (0, 1), False),
    "F_TO_CANONICAL": (8, 8, 8, (0, 1), False), "F_FROM_CANONICAL": (9, 8, 8, (0, 1), False), "F_FROM_U64": (10, 2, 8, (0, 1), False),
    "F_POW_U64": (11, 10, 8, (0, 1), False),
    "W_MULW": (20, 18, 9, (0, 1), False), "W_MULW2": (21, 36, 18, (0, 1), False), "W_SQRW": (22, 9, 9, (0, 1), False),
    "W_SQRW2": (23, 18, 18, (0, 1), False), "W_MUL2ADDW": (24, 36, 9, (0, 1), False), "W_MULSUM3W": (25, 54, 9, (0, 1), False),
    "W_MUL_TW3": (26, 36, 9, (0, 1), False), "W_MUL_TW3_2": (27, 45, 18, (0, 1), False), "W_MULW_OS": (28, 18, 9, (0, 1), False),
    "W_SQRW_OS": (29, 9, 9, (0, 1), False), "W_MUL2ADDW_OS": (30, 36, 9, (0, 1), False),
    "W_SUB2": (31, 18, 9, (0, 1), False), "W_SUB4": (32, 18, 9, (0, 1), False), "W_SUB6": (33, 18, 9, (0, 1), False),
    "W_NEG2": (34, 9, 9, (0, 1), False), "W_NORMW": (35, 9, 9, (0, 1), False), "W_CSUB_P": (36, 9, 9, (0, 1), False),
    "W_REDUCE_FULL": (37, 9, 9, (0, 1), False), "W_REDUCE_SMALL": (38, 9, 9, (0, 1), False), "W_IS_ZERO_MOD_P": (39, 9, 1, (0, 1), False),
    "W_MAYBE_ZERO_MOD_P": (40, 9, 1, (0, 1), False), "W_UNPACK": (41, 8, 9, (0, 1), False), "W_PACK": (42, 9, 8, (0, 1), False),
    "W_W_FROM_S": (43, 9, 9, (0, 1), False), "W_S_FROM_W": (44, 9, 9, (0, 1), False),
    "E_XYZZ_ADD_MIXED": (60, 49, 32, (1,), False), "E_XYZZ_ADD": (61, 64, 32, (1,), False), "E_XYZZ_DOUBLE": (62, 32, 32, (1,), False),
    "E_XYZZW_ADD_MIXED": (63, 55, 36, (1,), False), "E_XYZZW_ADD": (64, 72, 36, (1,), False), "E_XYZZW_DOUBLE": (65, 36, 36, (1,), False),
    "E_XYZZW_DOUBLE_AFFINE": (66, 18, 36, (1,), False), "E_XYZZW_ADD_MIXED_SPECIAL": (67, 73, 36, (1,), False),
    "E_XYZZW_CHAIN": (68, 140, 36 * CHAIN_STEPS, (1,), False), "E_XYZZW_ADD_MIXED_OS": (76, 55, 36, (1,), False),
    "E_XYZZW_EXPORT": (69, 36, 32, (1,), True), "E_XYZZW_STORE_LOAD": (70, 36, 72, (1,), True),
    "Q_ADD_DIST": (71, 72, 36, (1,), True),
    "Q_DISTRIBUTE_GATHER0": (72, 144, 144, (1,), True), "Q_DISTRIBUTE_GATHER1": (73, 144, 144, (1,), True),
    "Q_DISTRIBUTE_GATHER2": (74, 144, 144, (1,), True), "Q_DISTRIBUTE_GATHER3": (75, 144, 144, (1,), True),
    "G_GLV_SPLIT": (80, 8, 12, (0,), False), "G_GLV_DIGITS": (81, 5, 6, (0,), False), "G_GLV_DIGITS4": (82, 5, 6, (0,), False),
    "G_RECODE17": (83, 8, 15, (0,), False), "G_EXTRACT_BITS": (84, 10, 1, (0,), False),
    # g1_mul_dev.h: an XyzzW base (Fq) and a canonical Fr scalar; filed under Fq like the other point operations
    "G_MUL_SCALAR": (85, 44, 36, (1,), True), "G_MUL_SCALAR_ISO": (86, 44, 36, (1,), True), "G_MUL_SCALAR_ISO8": (87, 44, 36, (1,), True),
}
MUL_OPS = ("G_MUL_SCALAR", "G_MUL_SCALAR_ISO", "G_MUL_SCALAR_ISO8")


# ------------------------------------------------------------------------------------ limbs <-> integers
def w_int(l):
    return sum(int(v) << (29 * i) for i, v in enumerate(l))


def f_int(l):
    return sum(int(v) << (32 * i) for i, v in enumerate(l))


def int_w(v):
    """normalised 9 x 29-bit limbs; whatever is above 2^232 stays in the top limb"""
    assert 0 <= v < 1 << (232 + 32)
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def int_f(v, n=8):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def lazy_w(v):
    """the same integer with every limb but the top one pushed into [2^29, 2^30) where the limb above can lend"""
    l = int_w(v)
    for i in range(8):
        if l[i + 1] > 0:
            l[i] += 1 << 29
            l[i + 1] -= 1
    assert w_int(l) == v and max(l) < 1 << 30
    return l


def mont(t, p, bits):
    """(t + m p) >> bits with m = -t p^-1 mod 2^bits: the unique Montgomery reduction of the integer t"""
    m = (-t * pow(p, -1, 1 << bits)) % (1 << bits)
    assert (t + m * p) % (1 << bits) == 0
    return (t + m * p) >> bits


def hexw(l):
    return "[" + " ".join("%x" % v for v in l) + "]"


class Group:
    def __init__(self, name, field):
        self.name, self.field = name, field
        self.op, self.in_w, self.out_w, _, self.device_only = OPS[name]
        self.cases = []          # flat input words
        self.meta = []           # what the checker needs beyond the words (expected points)

    def add(self, words, meta=None):
        assert len(words) == self.in_w, (self.name, len(words))
        assert all(0 <= w < 1 << 32 for w in words), self.name
        self.cases.append(list(words))
        self.meta.append(meta)


# ------------------------------------------------------------------------------------ directed values
def edge_values(p):
    """normalised values below p that sit on limb boundaries of both layers, and the constants of both Montgomery radices"""
    top = p >> 232
    e = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R256 % p, (p - 1) * R256 % p, R261 % p, (p - 1) * R261 % p]
    for k in range(1, 9):
        e += [v for v in ((1 << (29 * k)), (1 << (29 * k)) - 1) if v < p]
    for k in range(1, 8):
        e += [v for v in ((1 << (32 * k)), (1 << (32 * k)) - 1) if v < p]
    e.append(((top - 1) << 232) | ((1 << 232) - 1))                       # every limb 2^29 - 1, the top one as large as stays below p
    e += [M29 << (29 * i) for i in range(8)] + [(top - 1) << 232]            # one limb at its maximum, the others zero
    e.append((R256 - 1) % p)                                              # eight 32-bit limbs of 0xffffffff, reduced
    e += [(0xffffffff << (32 * i)) % p for i in range(8)]
    out = []
    for v in e:
        assert 0 <= v < p
        if v not in out:
            out.append(v)
    return out


ALL_M29 = [M29] * 9                                                       # 2^261 - 1: the largest normalised vector


def rand_norm(rng, bound):
    return int_w(rng.randrange(bound))


# ------------------------------------------------------------------------------------ BN254 G1, affine, plain integers
def ec_add(a, b):
    q = Q_MOD
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % q == 0:
            return None
        s = 3 * a[0] * a[0] * pow(2 * a[1], -1, q) % q
    else:
        s = (b[1] - a[1]) * pow(b[0] - a[0], -1, q) % q
    x = (s * s - a[0] - b[0]) % q
    return (x, (s * (a[0] - x) - a[1]) % q)


def ec_neg(a):
    return None if a is None else (a[0], (-a[1]) % Q_MOD)


_MULTIPLES = [None, (1, 2)]


def multiple(k):
    """k * (1, 2) for small k (negative k: the opposite point; 0: infinity)"""
    if k < 0:
        return ec_neg(multiple(-k))
    while len(_MULTIPLES) <= k:
        _MULTIPLES.append(ec_add(_MULTIPLES[-1], (1, 2)))
    return _MULTIPLES[k]


_FIXED_BASE = []                        # [i][j] = j * 256^i * (1, 2), j = 0 .. 255


def g_mul(k):
    """(k mod r) * (1, 2) by the affine group law above: one table look-up and one ec_add per byte of k"""
    k %= R_MOD
    if not _FIXED_BASE:
        b = (1, 2)
        for _ in range(32):
            row = [None, b]
            for _ in range(254):
                row.append(ec_add(row[-1], b))
            _FIXED_BASE.append(row)
            b = ec_add(row[255], b)
    acc = None
    for i in range(32):
        acc = ec_add(acc, _FIXED_BASE[i][(k >> (8 * i)) & 255])
    return acc


def glv_split_model(k):
    """what glv_dev.h states glv_split computes, in integers: (|k1|, |k2|, k1 < 0, k2 < 0).  Only used to CHOOSE scalars with a given split; the
    expected result of a multiplication never depends on it"""
    g1, g2 = (GLV_B2 << 256) // R_MOD, (GLV_B1N << 256) // R_MOD
    c1, c2 = (k * g1) >> 256, (k * g2) >> 256
    k1, k2 = k - c1 * GLV_A1 - c2 * GLV_A2, c1 * GLV_B1N - c2 * GLV_B2
    assert (k1 + k2 * LAMBDA - k) % R_MOD == 0
    return abs(k1), abs(k2), k1 < 0, k2 < 0


def omega(log_n):
    """the generator of the size-2^log_n domain (Fr's multiplicative generator is 7)"""
    return pow(7, (R_MOD - 1) >> log_n, R_MOD)


def xyzz_words(pt, l, radix, i=0, j=0, zz_up=False, zzz_up=False, lazy=True):
    """(x l^2 + i q, y l^3 + j q, l^2 (+ q), l^3 (+ q)) in the Montgomery domain `radix`; None -> all zero.  lazy: 9 x 29-bit limbs, else 8 x 32"""
    q = Q_MOD
    conv = int_w if lazy else int_f
    if pt is None:
        return conv(0) * 4
    x = pt[0] * l * l % q * radix % q + i * q
    y = pt[1] * l * l * l % q * radix % q + j * q
    zz = l * l % q * radix % q
    zzz = l * l * l % q * radix % q
    if zz_up:
        assert 10 * zz < 3 * q
        zz += q
    if zzz_up:
        assert 10 * zzz < 3 * q
        zzz += q
    return conv(x) + conv(y) + conv(zz) + conv(zzz)


def aff_words(pt, radix, lazy=True):
    conv = int_w if lazy else int_f
    if pt is None:
        return conv(0) * 2
    return conv(pt[0] * radix % Q_MOD) + conv(pt[1] * radix % Q_MOD)


def decode_xyzz(words, radix, lazy=True):
    """-> (affine point or None, error string or None)"""
    q = Q_MOD
    n, val = (9, w_int) if lazy else (8, f_int)
    rinv = pow(radix, -1, q)
    X, Y, ZZ, ZZZ = (val(words[n * k:n * k + n]) * rinv % q for k in range(4))
    if ZZ == 0:
        return None, None
    if pow(ZZ, 3, q) != ZZZ * ZZZ % q:
        return None, "ZZ^3 != ZZZ^2"
    return (X * pow(ZZ, -1, q) % q, Y * pow(ZZZ, -1, q) % q), None


def check_xyzzw(words, want, what):
    """a lazy XYZZ result: the point, and the invariants at the top of ec29_dev.h (limbs normalised, x, y < 6p, zz, zzz < 1.3p)"""
    q = Q_MOD
    assert max(words) <= M29, "%s: limb not normalised: %s" % (what, hexw(words))
    x, y, zz, zzz = (w_int(words[9 * k:9 * k + 9]) for k in range(4))
    assert x < 6 * q and y < 6 * q, "%s: x = %.3f p, y = %.3f p (bound 6p)" % (what, x / q, y / q)
    assert 10 * zz < 13 * q and 10 * zzz < 13 * q, "%s: zz = %.3f p, zzz = %.3f p (bound 1.3p)" % (what, zz / q, zzz / q)
    got, err = decode_xyzz(words, R261)
    assert err is None, "%s: %s" % (what, err)
    if want is None:
        assert zz == 0, "%s: expected infinity (zz limbs all zero), zz = %x" % (what, zz)
    else:
        assert zz % q != 0, "%s: got infinity, expected %s" % (what, want)
    assert got == want, "%s: point %s, expected %s" % (what, got, want)


def check_xyzz(words, want, what):
    q = Q_MOD
    vals = [f_int(words[8 * k:8 * k + 8]) for k in range(4)]
    assert max(vals) < q, "%s: coordinate not canonical" % what
    got, err = decode_xyzz(words, R256, lazy=False)
    assert err is None, "%s: %s" % (what, err)
    if want is None:
        assert vals[2] == 0, "%s: expected infinity" % what
    assert got == want, "%s: point %s, expected %s" % (what, got, want)


# ------------------------------------------------------------------------------------ checkers: (p, in words, out words, meta) -> raise
def _fp_checker(fn):
    def chk(p, i, o, meta):
        want = fn(p, i)
        assert f_int(o) == want, "got %x, expected %x" % (f_int(o), want)
    return chk


def _rinv(p):
    return pow(R256, -1, p)


def _exact_w(fn, all_limbs=False):
    """exact integer value; limbs 0..7 normalised (all nine where the header promises a value below 2^261)"""
    def chk(p, i, o, meta):
        wants = fn(p, i)
        wants = wants if isinstance(wants, tuple) else (wants,)
        for k, want in enumerate(wants):
            got = o[9 * k:9 * k + 9]
            assert max(got[:8]) <= M29, "a limb below the top one is not below 2^29: %s" % hexw(got)
            if all_limbs:
                assert got[8] <= M29, "top limb not below 2^29: %s" % hexw(got)
            assert w_int(got) == want, "result %d: got %x, expected %x" % (k, w_int(got), want)
    return chk


def _w(i, k):
    return w_int(i[9 * k:9 * k + 9])


def _tw3(p, i, xo, to):
    x = i[xo:xo + 9]
    t = sum(w_int(x[3 * c:3 * c + 3]) * w_int(i[to + 9 * c:to + 9 * c + 9]) for c in range(3))
    return mont(t, p, 87)


def _chk_is_zero(p, i, o, meta):
    assert o[0] == (1 if _w(i, 0) % p == 0 else 0), "got %d for a value that is %s mod p" % (o[0], "0" if _w(i, 0) % p == 0 else "not 0")


def _chk_maybe_zero(p, i, o, meta):
    assert o[0] in (0, 1)
    if _w(i, 0) % p == 0:
        assert o[0] == 1, "false negative: the value is a multiple of p"


_exact_w_from_s = _exact_w(lambda p, i: mont(_w(i, 0) * (R261 * 32 % p), p, 261), all_limbs=True)    # x 2^256 -> x 2^261: the product by 2^266 mod p


def _chk_w_from_s(p, i, o, meta):
    _exact_w_from_s(p, i, o, meta)
    assert 10 * w_int(o) < 11 * p, "result %.3f p, documented below 1.1 p" % (w_int(o) / p)


def _chk_unpack(p, i, o, meta):
    assert max(o) <= M29 and w_int(o) == f_int(i), "got %s" % hexw(o)


def _chk_pack(p, i, o, meta):
    assert f_int(o) == w_int(i), "got %x" % f_int(o)


def _chk_glv_split(p, i, o, meta):
    k = f_int(i)
    k1, k2 = f_int(o[0:5]), f_int(o[5:10])
    assert o[10] in (0, 1) and o[11] in (0, 1)
    assert k1 < 1 << 127 and k2 < 1 << 127, "halves %x %x not below 2^127" % (k1, k2)
    assert ((-k1 if o[10] else k1) + (-k2 if o[11] else k2) * LAMBDA - k) % R_MOD == 0, "k1 %x neg %d k2 %x neg %d" % (k1, o[10], k2, o[11])


def _digits_checker(windows, bits, per_word, lo, hi):
    """codes of bits + 1 bits (top bit: negative, the rest: magnitude), per_word to a word, low window first: they re-sum to the magnitude"""
    def chk(p, i, o, meta):
        k, total, used = f_int(i), 0, [0] * 6
        for w in range(windows):
            shift = (bits + 1) * (w % per_word)
            code = (o[w // per_word] >> shift) & ((2 << bits) - 1)
            used[w // per_word] |= ((2 << bits) - 1) << shift
            d = (code & ((1 << bits) - 1)) * (-1 if code >> bits else 1)
            assert lo <= d <= hi, "digit %d of window %d outside [%d, %d]" % (d, w, lo, hi)
            total += d * (1 << (bits * w))
        assert all(o[n] & ~used[n] == 0 for n in range(6)), "bits set outside the digit codes"
        assert total == k, "digits sum to %x, expected %x" % (total, k)
    return chk


def _chk_recode17(p, i, o, meta):
    k = f_int(i)
    d = [v - (1 << 32) if v >> 31 else v for v in o]
    for w in range(14):
        assert -(1 << 16) <= d[w] <= 1 << 16, "window %d digit %d outside [-2^16, 2^16]" % (w, d[w])
    assert d[14] >= 0, "top window digit %d is negative" % d[14]
    total = sum(v << (17 * w) for w, v in enumerate(d))
    assert total == k, "digits %s sum to %x, expected %x" % (d, total, k)


def _chk_extract_bits(p, i, o, meta):
    k, pos, c = f_int(i[:8]), i[8], i[9]
    want = (k >> pos) & ((1 << c) - 1)
    assert o[0] == want, "pos %d c %d: got %x, expected %x" % (pos, c, o[0], want)


def _chk_point_w(p, i, o, meta):
    check_xyzzw(o, meta, "result")


def _chk_point_s(p, i, o, meta):
    check_xyzz(o, meta, "result")


def _chk_chain(p, i, o, meta):
    for s, want in enumerate(meta):
        check_xyzzw(o[36 * s:36 * s + 36], want, "step %d of schedule %s" % (s, i[108:108 + CHAIN_STEPS]))


def _chk_export(p, i, o, meta):
    if max(i[18:27]) == 0:
        assert max(o) == 0, "infinity must export as all zero"
        return
    for k in range(4):
        want = w_int(i[9 * k:9 * k + 9]) * R256 % p * pow(R261, -1, p) % p
        assert f_int(o[8 * k:8 * k + 8]) == want, "coordinate %d: got %x, expected %x" % (k, f_int(o[8 * k:8 * k + 8]), want)


def _chk_store_load(p, i, o, meta):
    assert o[:36] == i, "load_xyzzw(store_xyzzw(v)) != v: %s" % hexw(o[:36])
    image = [i[9 * k + l] for k in range(4) for l in range(8)] + [i[9 * k + 8] for k in range(4)]     # 4 x 8 limbs, then the four 9th limbs
    assert o[36:] == image, "memory image %s, expected %s" % (hexw(o[36:]), hexw(image))


def _chk_gather(p, i, o, meta):
    for lane in range(4):
        assert o[36 * lane:36 * lane + 36] == i[36 * meta:36 * meta + 36], "lane %d did not receive lane %d's point" % (lane, meta)


_MULW = _exact_w(lambda p, i: mont(_w(i, 0) * _w(i, 1), p, 261))
_SQRW = _exact_w(lambda p, i: mont(_w(i, 0) ** 2, p, 261))
_MUL2ADDW = _exact_w(lambda p, i: mont(_w(i, 0) * _w(i, 1) + _w(i, 2) * _w(i, 3), p, 261))
_CANONICAL = _exact_w(lambda p, i: _w(i, 0) % p, all_limbs=True)
CHECKERS = {
    "F_ADD": _fp_checker(lambda p, i: (f_int(i[:8]) + f_int(i[8:])) % p),
    "F_SUB": _fp_checker(lambda p, i: (f_int(i[:8]) - f_int(i[8:])) % p),
    "F_NEG": _fp_checker(lambda p, i: -f_int(i) % p),
    "F_DBL": _fp_checker(lambda p, i: 2 * f_int(i) % p),
    "F_MUL": _fp_checker(lambda p, i: f_int(i[:8]) * f_int(i[8:]) * _rinv(p) % p),
    "F_SQR": _fp_checker(lambda p, i: f_int(i) ** 2 * _rinv(p) % p),
    "F_INV": _fp_checker(lambda p, i: 0 if f_int(i) == 0 else pow(f_int(i), -1, p) * R256 * R256 % p),
    "F_TO_CANONICAL": _fp_checker(lambda p, i: f_int(i) * _rinv(p) % p),
    "F_FROM_CANONICAL": _fp_checker(lambda p, i: f_int(i) * R256 % p),
    "F_FROM_U64": _fp_checker(lambda p, i: f_int(i) * R256 % p),
    "F_POW_U64": _fp_checker(lambda p, i: pow(f_int(i[:8]) * _rinv(p), f_int(i[8:]), p) * R256 % p),
    "W_MULW": _MULW, "W_MULW_OS": _MULW,
    "W_MULW2": _exact_w(lambda p, i: (mont(_w(i, 0) * _w(i, 1), p, 261), mont(_w(i, 2) * _w(i, 3), p, 261))),
    "W_SQRW": _SQRW, "W_SQRW_OS": _SQRW,
    "W_SQRW2": _exact_w(lambda p, i: (mont(_w(i, 0) ** 2, p, 261), mont(_w(i, 1) ** 2, p, 261))),
    "W_MUL2ADDW": _MUL2ADDW, "W_MUL2ADDW_OS": _MUL2ADDW,
    "W_MULSUM3W": _exact_w(lambda p, i: mont(_w(i, 0) * _w(i, 1) + _w(i, 2) * _w(i, 3) + _w(i, 4) * _w(i, 5), p, 261)),
    "W_MUL_TW3": _exact_w(lambda p, i: _tw3(p, i, 0, 9)),
    "W_MUL_TW3_2": _exact_w(lambda p, i: (_tw3(p, i, 0, 18), _tw3(p, i, 9, 18))),
    "W_SUB2": _exact_w(lambda p, i: _w(i, 0) + 2 * p - _w(i, 1), all_limbs=True),
    "W_SUB4": _exact_w(lambda p, i: _w(i, 0) + 4 * p - _w(i, 1), all_limbs=True),
    "W_SUB6": _exact_w(lambda p, i: _w(i, 0) + 6 * p - _w(i, 1), all_limbs=True),
    "W_NEG2": _exact_w(lambda p, i: 2 * p - _w(i, 0), all_limbs=True),
    "W_NORMW": _exact_w(lambda p, i: _w(i, 0), all_limbs=True),
    "W_CSUB_P": _CANONICAL, "W_REDUCE_FULL": _CANONICAL, "W_REDUCE_SMALL": _CANONICAL,
    "W_IS_ZERO_MOD_P": _chk_is_zero,
    "W_MAYBE_ZERO_MOD_P": _chk_maybe_zero,
    "W_UNPACK": _chk_unpack,
    "W_PACK": _chk_pack,
    "W_W_FROM_S": _chk_w_from_s,
    "W_S_FROM_W": _exact_w(lambda p, i: _w(i, 0) * R256 % p * pow(R261, -1, p) % p, all_limbs=True),
    "E_XYZZ_ADD_MIXED": _chk_point_s, "E_XYZZ_ADD": _chk_point_s, "E_XYZZ_DOUBLE": _chk_point_s,
    "E_XYZZW_ADD_MIXED": _chk_point_w, "E_XYZZW_ADD": _chk_point_w, "E_XYZZW_DOUBLE": _chk_point_w, "E_XYZZW_DOUBLE_AFFINE": _chk_point_w,
    "E_XYZZW_ADD_MIXED_SPECIAL": _chk_point_w, "E_XYZZW_ADD_MIXED_OS": _chk_point_w, "E_XYZZW_CHAIN": _chk_chain, "E_XYZZW_EXPORT": _chk_export, "E_XYZZW_STORE_LOAD": _chk_store_load,
    "Q_ADD_DIST": _chk_point_w,
    "Q_DISTRIBUTE_GATHER0": _chk_gather, "Q_DISTRIBUTE_GATHER1": _chk_gather, "Q_DISTRIBUTE_GATHER2": _chk_gather, "Q_DISTRIBUTE_GATHER3": _chk_gather,
    "G_GLV_SPLIT": _chk_glv_split,
    "G_GLV_DIGITS": _digits_checker(43, 3, 8, -3, 4),
    "G_GLV_DIGITS4": _digits_checker(32, 4, 6, -7, 8),
    "G_RECODE17": _chk_recode17,
    "G_EXTRACT_BITS": _chk_extract_bits,
    # k * b; the result goes straight into the stage's xyzzw_add, so it must meet that function's operand contract: the same checks
    "G_MUL_SCALAR": _chk_point_w, "G_MUL_SCALAR_ISO": _chk_point_w, "G_MUL_SCALAR_ISO8": _chk_point_w,
}
assert sorted(CHECKERS) == sorted(OPS)


def describe_inputs(g, words):
    if g.name in MUL_OPS:
        return " | ".join(hexw(words[k:k + 9]) for k in range(0, 36, 9)) + " | scalar %x" % f_int(words[36:])
    if g.name[0] in "FG" or g.name.startswith("E_XYZZ_"):
        return hexw(words)
    return " | ".join(hexw(words[k:k + 9]) for k in range(0, len(words), 9))


def check_group(g, outs):
    """every case of the group against the integer model; returns the number of cases checked"""
    assert len(outs) == len(g.cases), "%s<%s>: %d cases generated, %d results" % (g.name, FIELD_NAME[g.field], len(g.cases), len(outs))
    chk, p, n = CHECKERS[g.name], MOD[g.field], 0
    for idx, (i, o, meta) in enumerate(zip(g.cases, outs, g.meta)):
        try:
            chk(p, i, o, meta)
        except AssertionError as e:
            raise AssertionError("%s<%s> case %d: %s\n  operands: %s\n  result:   %s"
                                 % (g.name, FIELD_NAME[g.field], idx, e, describe_inputs(g, i), hexw(o))) from None
        n += 1
    return n


# ------------------------------------------------------------------------------------ the cases
def _field_groups(fld, rng):
    p = MOD[fld]
    E = edge_values(p)
    groups = []

    def grp(name):
        g = Group(name, fld)
        groups.append(g)
        return g

    # ---- 8 x 32-bit Montgomery layer: reduced operands, the whole cross product of the edge list (it holds x and p - x for several x: the ties
    # of the final conditional subtraction, t == p), and uniform ones
    def rf():
        return int_f(rng.randrange(p))
    for name in ("F_ADD", "F_SUB", "F_MUL"):
        g = grp(name)
        for a, b in itertools.product(E, E):
            g.add(int_f(a) + int_f(b))
        for _ in range(RANDOM_CASES):
            g.add(rf() + rf())
    for name in ("F_NEG", "F_DBL", "F_SQR", "F_INV", "F_TO_CANONICAL", "F_FROM_CANONICAL"):
        g = grp(name)
        for a in E:
            g.add(int_f(a))
        for _ in range(RANDOM_CASES):
            g.add(rf())
    g = grp("F_FROM_U64")
    u64_edges = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63), (1 << 64) - 1, (1 << 64) - 2, 0xffffffff00000000]
    for v in u64_edges:
        g.add(int_f(v, 2))
    for _ in range(RANDOM_CASES):
        g.add(int_f(rng.randrange(1 << 64), 2))
    g = grp("F_POW_U64")
    for a, e in itertools.product(E, u64_edges):
        g.add(int_f(a) + int_f(e, 2))
    for _ in range(RANDOM_CASES):
        g.add(rf() + int_f(rng.randrange(1 << rng.choice((1, 8, 33, 64))), 2))

    # ---- 9 x 29-bit lazy layer
    norm_edges = [int_w(v) for v in E] + [ALL_M29]
    # mulw's LEFT operand up to its documented limits: limbs at MULW_A_LIMB_MAX, the raw sums the kernels feed in (x + PAD2 - y, x + y).
    # PAD2 is 2p with its lower limbs biased by 2^31, each bias taken back as 4 from the limb above (field29_dev.h: "PADk")
    n2p = int_w(2 * p)
    pad2 = [n2p[0] + (1 << 31)] + [n2p[i] + (1 << 31) - 4 for i in range(1, 8)] + [n2p[8] - 4]
    assert w_int(pad2) == 2 * p
    left_lazy = [[MULW_A_LIMB_MAX] * 9]
    left_lazy += [[MULW_A_LIMB_MAX if i == k else 0 for i in range(9)] for k in range(9)]
    for x, y in ((ALL_M29, int_w(0)), (int_w(p - 1), int_w(p - 1)), (int_w(0), [M29] * 8 + [pad2[8]]), (int_w(E[5]), int_w(E[6]))):
        left_lazy.append([x[i] + pad2[i] - y[i] for i in range(9)])
        left_lazy.append([x[i] + y[i] for i in range(9)])
    left = norm_edges + left_lazy
    assert all(0 <= min(l) and max(l) <= MULW_A_LIMB_MAX for l in left)

    def rand_left():
        kind = rng.randrange(4)
        if kind == 0:
            return rand_norm(rng, p)
        if kind == 1:
            return rand_norm(rng, R261)
        if kind == 2:
            return [rng.randrange(MULW_A_LIMB_MAX + 1) for _ in range(9)]
        x, y = rand_norm(rng, R261), rand_norm(rng, 2 * p - (4 << 232))
        return [x[i] + pad2[i] - y[i] for i in range(9)]

    def rand_right():
        return rand_norm(rng, p if rng.randrange(2) else R261)
    for name in ("W_MULW", "W_MULW_OS"):
        g = grp(name)
        for a, b in itertools.product(left, norm_edges):
            g.add(a + b)
        for _ in range(RANDOM_CASES):
            g.add(rand_left() + rand_right())
    g = grp("W_MULW2")                                           # two independent products in lockstep: every directed pair, next to another one
    pairs = [a + b for a, b in itertools.product(left, norm_edges)]
    for k, ab in enumerate(pairs):
        g.add(ab + pairs[(k * 7 + 13) % len(pairs)])
    for _ in range(RANDOM_CASES):
        g.add(rand_left() + rand_right() + rand_left() + rand_right())
    for name in ("W_SQRW", "W_SQRW_OS"):                       # normalised input (ec29_dev.h: WS)
        g = grp(name)
        for a in norm_edges:
            g.add(a)
        for _ in range(RANDOM_CASES):
            g.add(rand_right())
    g = grp("W_SQRW2")
    for a, b in itertools.product(norm_edges, norm_edges):
        g.add(a + b)
    for _ in range(RANDOM_CASES):
        g.add(rand_right() + rand_right())
    # a*b + c*d: a, c limbs just below 2^30; b, d normalised.  Four operand positions: the cross product of eight values each
    ac = [int_w(0), int_w(1), int_w(p - 1), ALL_M29, [(1 << 30) - 1] * 9, int_w(R261 % p), [(1 << 30) - 1] + [0] * 8, [0] * 8 + [(1 << 30) - 1]]
    bd = [int_w(0), int_w(1), int_w(p - 1), ALL_M29, int_w(1 << 116), int_w((p - 1) // 2), int_w(R261 % p), [0] * 7 + [M29, 0]]
    for name in ("W_MUL2ADDW", "W_MUL2ADDW_OS"):
        g = grp(name)
        for a, b, c, d in itertools.product(ac, bd, ac, bd):
            g.add(a + b + c + d)
        for _ in range(RANDOM_CASES):
            g.add([rng.randrange(1 << 30) for _ in range(9)] + rand_right() + [rng.randrange(1 << 30) for _ in range(9)] + rand_right())
    g = grp("W_MULSUM3W")                                        # normalised inputs; six positions: the cross product of four values each
    four = [int_w(0), int_w(1), int_w(p - 1), ALL_M29]
    for ops in itertools.product(four, repeat=6):
        g.add([w for o in ops for w in o])
    for _ in range(RANDOM_CASES):
        g.add([w for _ in range(6) for w in rand_right()])

    # product by a constant held as three shifted copies W_q = w 2^(87 (q + 1)) mod p (canonical): x limbs up to MULTW3_X_LIMB_MAX
    def tw3(w):
        return [l for c in range(3) for l in int_w(w * pow(2, 87 * (c + 1), p) % p)]
    consts = [tw3(w) for w in (0, 1, 2, p - 1, (p - 1) // 2, R261 % p, (p - 1) * R261 % p)] + [tw3(rng.randrange(p)) for _ in range(3)]
    xs = norm_edges + [[MULTW3_X_LIMB_MAX] * 9] + [[MULTW3_X_LIMB_MAX if i == k else 0 for i in range(9)] for k in range(9)]
    raw_max = [M29] * 27                                         # no constant anybody builds, but inside "W < 2^29"; with normalised x only

    def rand_x():
        return [rng.randrange(MULTW3_X_LIMB_MAX + 1) for _ in range(9)] if rng.randrange(3) == 0 else rand_norm(rng, R261)
    g = grp("W_MUL_TW3")
    for x, t in itertools.product(xs, consts):
        g.add(x + t)
    for x in norm_edges:
        g.add(x + raw_max)
    for _ in range(RANDOM_CASES):
        g.add(rand_x() + tw3(rng.randrange(p)))
    g = grp("W_MUL_TW3_2")
    for k, (x, t) in enumerate(itertools.product(xs, consts)):
        g.add(x + xs[(k * 5 + 3) % len(xs)] + t)
    for _ in range(RANDOM_CASES):
        g.add(rand_x() + rand_x() + tw3(rng.randrange(p)))
    # a - b + k p: b below k p with limbs below 2^30; a: limbs below 2^30, a + k p below 2^261
    for k, name in ((2, "W_SUB2"), (4, "W_SUB4"), (6, "W_SUB6")):
        g = grp(name)
        a_list = [int_w(v) for v in E] + [int_w(R261 - 1 - 8 * p), lazy_w(R261 - 1 - 8 * p), [(1 << 30) - 1] * 8 + [0], int_w(k * p - 1), lazy_w(k * p - 1)]
        b_list = [int_w(v) for v in E] + [int_w(k * p - 1), lazy_w(k * p - 1), lazy_w(k * p - 2), int_w((k - 1) * p), lazy_w((k - 1) * p + 1), lazy_w(p), int_w(p)]
        assert all(w_int(b) < k * p and max(b) < 1 << 30 for b in b_list)
        for a, b in itertools.product(a_list, b_list):
            g.add(a + b)
        for b in b_list:                                         # b == a
            g.add(b + b)
        for _ in range(RANDOM_CASES):
            v = rng.randrange(k * p)
            g.add(rand_norm(rng, R261 - 8 * p) + (lazy_w(v) if rng.randrange(2) else int_w(v)))
    g = grp("W_NEG2")
    for v in E + [p, p + 1, 2 * p - 1, 2 * p - 2]:
        g.add(int_w(v))
        g.add(lazy_w(v))
    for _ in range(RANDOM_CASES):
        v = rng.randrange(2 * p)
        g.add(lazy_w(v) if rng.randrange(2) else int_w(v))
    # carry propagation: limbs up to 2^32 - 8 (such a limb plus the largest carry, 7, is the last sum that fits 32 bits), value below 2^261
    g = grp("W_NORMW")
    big = (1 << 32) - 8
    for a in norm_edges + left_lazy + [[big] * 8 + [0], [big] * 8 + [M29 - 8]] + [[big if i == k else 0 for i in range(9)] for k in range(8)]:
        if w_int(a) < R261:
            g.add(a)
    for _ in range(RANDOM_CASES):
        g.add([rng.randrange(big + 1) for _ in range(8)] + [rng.randrange(M29 - 8)])
    g = grp("W_CSUB_P")                                          # normalised, below 2p
    for v in E + [v + p for v in E] + [p, p + 1, 2 * p - 1]:
        g.add(int_w(v))
    for _ in range(RANDOM_CASES):
        g.add(rand_norm(rng, 2 * p))
    g = grp("W_REDUCE_FULL")                                     # normalised, below 2^261
    for a in norm_edges:
        g.add(a)
    for k in list(range(0, 20)) + [63, 64, 100, 169]:
        for d in (-1, 0, 1):
            if 0 <= k * p + d < R261:
                g.add(int_w(k * p + d))
    for _ in range(RANDOM_CASES):
        g.add(rand_norm(rng, R261))
    g = grp("W_REDUCE_SMALL")                                    # normalised, below 64p
    for v in E:
        g.add(int_w(v))
    for k in range(64):
        for d in (-1, 0, 1):
            if 0 <= k * p + d:
                g.add(int_w(k * p + d))
        g.add(int_w((k * (p >> 232)) << 232))                    # the top limb alone says k p, the limbs below say less
    g.add(int_w(64 * p - 1))
    for _ in range(RANDOM_CASES):
        g.add(rand_norm(rng, 64 * p))
    # zero tests: normalised, below 16p.  That is all the header promises, so 16p itself is not asked.
    zero_cases = [int_w(v) for v in E]
    for k in range(16):
        zero_cases.append(int_w(k * p))                          # true zeros
        zero_cases.append(int_w(k * p + 1))
        for t in (1, 2, 3):
            if k * p + (t << 29) < 16 * p:
                zero_cases.append(int_w(k * p + (t << 29)))      # passes the cheap filter (limb 0 is that of k p), is not zero
    zero_cases.append(int_w(16 * p - 1))
    for _ in range(RANDOM_CASES):
        kind = rng.randrange(4)
        if kind == 0:
            zero_cases.append(int_w(rng.randrange(16) * p))
        elif kind == 1:
            v = rng.randrange(15 * p)
            zero_cases.append(int_w(v - (v & M29) + ((rng.randrange(16) * p) & M29)))      # limb 0 forged, the rest uniform
        else:
            zero_cases.append(rand_norm(rng, 16 * p))
    for name in ("W_IS_ZERO_MOD_P", "W_MAYBE_ZERO_MOD_P"):
        g = grp(name)
        for a in zero_cases:
            g.add(a)
    g = grp("W_UNPACK")
    bits256 = E + [R256 - 1, R256 - 2] + [1 << b for b in range(256) if b % 29 in (0, 28) or b % 32 in (0, 31)]
    for v in bits256:
        g.add(int_f(v))
    for _ in range(RANDOM_CASES):
        g.add(int_f(rng.randrange(R256)))
    g = grp("W_PACK")                                            # normalised, below 2^256
    for v in bits256:
        g.add(int_w(v))
    for _ in range(RANDOM_CASES):
        g.add(rand_norm(rng, R256))
    g = grp("W_W_FROM_S")                                        # the raw 256-bit external form, re-sliced
    for v in bits256:
        g.add(int_w(v))
    for _ in range(RANDOM_CASES):
        g.add(rand_norm(rng, p if rng.randrange(2) else R256))
    g = grp("W_S_FROM_W")                                        # a value below 2^261 (the product must come out below 2p), limbs lazy or not
    for a in norm_edges + [lazy_w(v) for v in E] + [lazy_w(R261 - 1)]:
        g.add(a)
    for _ in range(RANDOM_CASES):
        v = rng.randrange(R261)
        g.add(lazy_w(v) if rng.randrange(2) else int_w(v))
    return groups


def _point_variants(rng, full=True):
    """XYZZ representations (2^261 domain) at the edges of the accumulator contract: (l, i, j, zz_up, zzz_up) with x = X l^2 + i q, y = Y l^3 + j q,
    zz, zzz canonical or, where that stays below 1.3 q, canonical + q"""
    q = Q_MOD
    out = []
    for l in (1, rng.randrange(2, q)):
        ups = [(False, False)]
        zz, zzz = l * l % q * R261 % q, l * l * l % q * R261 % q
        if 10 * zz < 3 * q:
            ups.append((True, False))
        if 10 * zzz < 3 * q:
            ups.append((False, True))
        if 10 * zz < 3 * q and 10 * zzz < 3 * q:
            ups.append((True, True))
        ij = list(itertools.product(range(6), range(6))) if full else [(0, 0), (5, 5), (5, 0), (0, 5), (2, 3)]
        for (i, j), (u1, u2) in itertools.product(ij, ups):
            out.append((l, i, j, u1, u2))
    return out


def _curve_groups(rng, device):
    q = Q_MOD
    groups = []

    def grp(name):
        g = Group(name, 1)
        groups.append(g)
        return g
    ks = [1, 2, 3, 4, 5, 7, 8, 11, 16, 17, 29, 31, 32, 33, 64, 100, 127, 128, 255, 256, 300, 500]
    pair_list = [(1, 2), (2, 1), (3, 5), (7, 11), (16, 17), (127, 128), (255, 300), (500, 1), (5, 5), (1, 1), (33, 33), (256, 256)]
    pt = multiple

    def xw(k, var):
        l, i, j, u1, u2 = var
        return xyzz_words(pt(k), l, R261, i, j, u1, u2)

    def rand_var():
        return (rng.randrange(1, q), rng.randrange(6), rng.randrange(6), False, False)
    inf_garbage = int_w(rng.randrange(q)) + int_w(rng.randrange(q)) + int_w(0) + int_w(rng.randrange(q))     # ZZ == 0 is what says infinity
    zero36 = [0] * 36

    # ---- mixed addition, both signs
    g = grp("E_XYZZW_ADD_MIXED")
    for ka, kb in pair_list:
        for var in _point_variants(rng):
            for neg in (0, 1):
                g.add(xw(ka, var) + aff_words(pt(kb), R261) + [neg], ec_add(pt(ka), pt(-kb) if neg else pt(kb)))
        for var in _point_variants(rng, full=False):             # the opposite point as the operand itself: infinity without neg_q, doubling with it
            for neg in (0, 1):
                g.add(xw(ka, var) + aff_words(pt(-kb), R261) + [neg], ec_add(pt(ka), pt(kb) if neg else pt(-kb)))
    for kb in ks:
        for neg in (0, 1):
            want = pt(-kb) if neg else pt(kb)
            g.add(zero36 + aff_words(pt(kb), R261) + [neg], want)                       # infinity + Q
            g.add(inf_garbage + aff_words(pt(kb), R261) + [neg], want)
            for var in _point_variants(rng, full=False):
                g.add(xw(kb, var) + aff_words(None, R261) + [neg], pt(kb))            # P + the affine (0, 0)
    for neg in (0, 1):
        g.add(zero36 + aff_words(None, R261) + [neg], None)
    for _ in range(RANDOM_CASES):
        ka, kb, neg = rng.randrange(1, 512), rng.randrange(1, 512), rng.randrange(2)
        g.add(xw(ka, rand_var()) + aff_words(pt(kb), R261) + [neg], ec_add(pt(ka), pt(-kb) if neg else pt(kb)))

    # ---- full addition (the same cases go through the four-lane form on the device)
    add_cases = []
    for ka, kb in pair_list + [(5, -5), (1, -1), (-33, 33), (300, -300)]:
        for va, vb in itertools.product(_point_variants(rng, full=False), _point_variants(rng, full=False)):
            add_cases.append((xw(ka, va) + xw(kb, vb), ec_add(pt(ka), pt(kb))))
    for k in ks:
        for var in _point_variants(rng, full=False):
            add_cases.append((zero36 + xw(k, var), pt(k)))
            add_cases.append((xw(k, var) + zero36, pt(k)))
            add_cases.append((inf_garbage + xw(k, var), pt(k)))
            add_cases.append((xw(k, var) + inf_garbage, pt(k)))
    add_cases.append((zero36 + zero36, None))
    add_cases.append((inf_garbage + inf_garbage, None))
    for _ in range(RANDOM_CASES):
        ka, kb = rng.randrange(1, 512), rng.randrange(1, 512)
        add_cases.append((xw(ka, rand_var()) + xw(kb, rand_var()), ec_add(pt(ka), pt(kb))))
    g = grp("E_XYZZW_ADD")
    for words, want in add_cases:
        g.add(words, want)

    # ---- doubling
    g = grp("E_XYZZW_DOUBLE")
    for k in ks:
        for var in _point_variants(rng):
            g.add(xw(k, var), ec_add(pt(k), pt(k)))
    g.add(zero36, None)
    g.add(inf_garbage, None)
    for _ in range(RANDOM_CASES):
        k = rng.randrange(1, 512) * rng.choice((1, -1))
        g.add(xw(k, rand_var()), ec_add(pt(k), pt(k)))
    g = grp("E_XYZZW_DOUBLE_AFFINE")                             # affine input: canonical (and + q where that stays below 1.1 q)
    for k in list(range(1, RANDOM_CASES + 1)) + [-k for k in range(1, 513)]:
        x, y = pt(k)[0] * R261 % q, pt(k)[1] * R261 % q
        g.add(int_w(x) + int_w(y), ec_add(pt(k), pt(k)))
        if 10 * x < q or 10 * y < q:
            g.add(int_w(x + q if 10 * x < q else x) + int_w(y + q if 10 * y < q else y), ec_add(pt(k), pt(k)))

    # ---- the slow path of the mixed addition, called directly.  p and r are only ever asked whether they vanish mod q.
    g = grp("E_XYZZW_ADD_MIXED_SPECIAL")

    def forged():                                                # passes maybe_zero_mod_p (limb 0 is that of a multiple of q below 16 q), is not zero
        return int_w(rng.randrange(15) * q + (rng.randrange(1, 4) << 29))

    def nonzero():
        return int_w(rng.randrange(1, 16) * q - 1 - rng.randrange(q - 1))
    for ka, kb in pair_list + [(5, -5), (300, -300)]:
        for var in _point_variants(rng, full=False):
            for neg in (0, 1):
                want = ec_add(pt(ka), pt(-kb) if neg else pt(kb))
                g.add(xw(ka, var) + aff_words(pt(kb), R261) + [neg] + forged() + rand_norm(rng, 16 * q), want)          # the filter's false positive
                g.add(xw(ka, var) + aff_words(pt(kb), R261) + [neg] + forged() + int_w(rng.randrange(16) * q), want)
    for k in ks:
        for var in _point_variants(rng, full=False):
            for neg in (0, 1):
                s = -1 if neg else 1
                # acc holds the same point as +-q: p and r vanish, the result is its double
                g.add(xw(s * k, var) + aff_words(pt(k), R261) + [neg] + int_w(rng.randrange(16) * q) + int_w(rng.randrange(16) * q), ec_add(pt(s * k), pt(s * k)))
                # acc holds the opposite point: p vanishes, r does not
                g.add(xw(-s * k, var) + aff_words(pt(k), R261) + [neg] + int_w(rng.randrange(16) * q) + nonzero(), None)
    for _ in range(RANDOM_CASES):
        ka, kb, neg = rng.randrange(1, 512), rng.randrange(1, 512), rng.randrange(2)
        g.add(xw(ka, rand_var()) + aff_words(pt(kb), R261) + [neg] + forged() + rand_norm(rng, 16 * q), ec_add(pt(ka), pt(-kb) if neg else pt(kb)))

    # ---- chains of 32 dependent operations, every intermediate result checked: the bounds must be closed under repeated use
    g = grp("E_XYZZW_CHAIN")
    for c in range(512):
        ka = 0 if c % 16 == 0 else rng.randrange(1, 512)
        k0, k1, kb = rng.randrange(1, 512), rng.randrange(1, 512), rng.randrange(1, 512)
        if c % 8 == 1:
            k0 = ka                                              # the first mixed addition may be a doubling
        va = rng.choice(_point_variants(rng))
        vb = rng.choice(_point_variants(rng, full=False))
        sched = [rng.randrange(6) for _ in range(CHAIN_STEPS)]
        if c % 32 == 2:
            sched = [0] * CHAIN_STEPS                            # what a bucket does: the same kind of addition over and over
        if c % 32 == 3:
            sched = [4] * CHAIN_STEPS
        if c % 32 == 4:
            sched = [5] * CHAIN_STEPS
        if c % 32 == 5:
            sched = [0, 1] * (CHAIN_STEPS // 2)                  # back and forth: every second result repeats
        acc, wants = pt(ka), []
        for o in sched:
            if o < 4:
                acc = ec_add(acc, pt((k1 if o & 2 else k0) * (-1 if o & 1 else 1)))
            elif o == 4:
                acc = ec_add(acc, acc)
            else:
                acc = ec_add(acc, pt(kb))
            wants.append(acc)
        g.add(xw(ka, va) + aff_words(pt(k0), R261) + aff_words(pt(k1), R261) + xw(kb, vb) + sched, wants)

    # ---- the 8 x 32-bit group law
    def xs(k, l):
        return xyzz_words(pt(k), l, R256, lazy=False)

    def affs(k):
        return aff_words(pt(k), R256, lazy=False)
    zero32 = [0] * 32
    g = grp("E_XYZZ_ADD_MIXED")
    for (ka, kb), neg in itertools.product(pair_list + [(5, -5), (300, -300)], (0, 1)):
        for l in (1, rng.randrange(2, q)):
            g.add(xs(ka, l) + affs(kb) + [neg], ec_add(pt(ka), pt(-kb) if neg else pt(kb)))
    for k, neg in itertools.product(ks, (0, 1)):
        g.add(zero32 + affs(k) + [neg], pt(-k) if neg else pt(k))
        g.add(xs(k, rng.randrange(1, q)) + [0] * 16 + [neg], pt(k))
    g.add(zero32 + [0] * 16 + [0], None)
    for _ in range(RANDOM_CASES):
        ka, kb, neg = rng.randrange(1, 512), rng.randrange(1, 512), rng.randrange(2)
        g.add(xs(ka, rng.randrange(1, q)) + affs(kb) + [neg], ec_add(pt(ka), pt(-kb) if neg else pt(kb)))
    g = grp("E_XYZZ_ADD")
    for ka, kb in pair_list + [(5, -5), (1, -1), (-33, 33), (300, -300)]:
        for la, lb in itertools.product((1, rng.randrange(2, q)), repeat=2):
            g.add(xs(ka, la) + xs(kb, lb), ec_add(pt(ka), pt(kb)))
    for k in ks:
        g.add(zero32 + xs(k, rng.randrange(1, q)), pt(k))
        g.add(xs(k, rng.randrange(1, q)) + zero32, pt(k))
    g.add(zero32 + zero32, None)
    for _ in range(RANDOM_CASES):
        ka, kb = rng.randrange(1, 512), rng.randrange(1, 512)
        g.add(xs(ka, rng.randrange(1, q)) + xs(kb, rng.randrange(1, q)), ec_add(pt(ka), pt(kb)))
    g = grp("E_XYZZ_DOUBLE")
    for k in ks:
        for l in (1, rng.randrange(2, q)):
            g.add(xs(k, l), ec_add(pt(k), pt(k)))
    g.add(zero32, None)
    for _ in range(RANDOM_CASES):
        k = rng.randrange(1, 512) * rng.choice((1, -1))
        g.add(xs(k, rng.randrange(1, q)), ec_add(pt(k), pt(k)))

    if device:
        g = grp("Q_ADD_DIST")                                    # one case per quad: the cases of the lane-wise addition
        for words, want in add_cases:
            g.add(words, want)
        points = [w[:36] for w, _ in add_cases] + [w[36:] for w, _ in add_cases]
        for src in range(4):
            g = grp("Q_DISTRIBUTE_GATHER%d" % src)
            for c in range(RANDOM_CASES):
                g.add([w for lane in range(4) for w in points[(4 * c + lane + 17 * src) % len(points)]], src)
        for name in ("E_XYZZW_EXPORT", "E_XYZZW_STORE_LOAD"):
            g = grp(name)
            for words in points[:RANDOM_CASES] + points[-RANDOM_CASES:] + [zero36, inf_garbage]:
                g.add(words)
    return groups


def _scalar_groups(rng):
    r = R_MOD
    groups = []

    def grp(name):
        g = Group(name, 0)
        groups.append(g)
        return g
    directed = [0, 1, r - 1, r - 2, LAMBDA, LAMBDA * LAMBDA % r, r - LAMBDA]
    for w in range(15):
        directed += [(1 << (17 * w)) - 1, 1 << (17 * w), (1 << (17 * w)) + (1 << 16), (1 << (17 * w + 16)) - 1]
    directed.append(sum(1 << (17 * w + 16) for w in range(15)))             # every window at 2^16: the carry runs through all fifteen
    directed.append(sum(((1 << 16) - 1) << (17 * w) for w in range(15)))     # every window at 2^16 - 1
    g = grp("G_GLV_SPLIT")                                       # canonical scalars below r
    for k in directed:
        if k < r:
            g.add(int_f(k))
    for _ in range(RANDOM_CASES):
        g.add(int_f(rng.randrange(r)))
    g = grp("G_RECODE17")                                        # fifteen 17-bit windows: any value below 2^255 (the top window is unsigned and keeps its carry)
    for k in directed + [(1 << 255) - 1, (1 << 254), (1 << 254) - 1]:
        g.add(int_f(k))
    for _ in range(RANDOM_CASES):
        g.add(int_f(rng.randrange(r if rng.randrange(2) else 1 << 255)))
    g = grp("G_EXTRACT_BITS")                                    # against Python shifts: windows that straddle limb 7, positions at and past bit 256
    values = [int_f(v) for v in (R256 - 1, r - 1, 1 << 255, int("a5" * 32, 16), rng.randrange(R256))]
    for v, pos, c in itertools.product(values, list(range(200, 300)) + [0, 1, 17, 31, 32, 33, 63, 64, 1000, 0xffffffff], (1, 13, 16, 17, 24, 31)):
        g.add(v + [pos, c])
    for _ in range(RANDOM_CASES):
        g.add(int_f(rng.randrange(R256)) + [rng.randrange(320), rng.randrange(1, 32)])
    for name, bits, lim in (("G_GLV_DIGITS", 3, 128), ("G_GLV_DIGITS4", 4, 127)):
        g = grp(name)                                            # magnitudes below 2^128 / 2^127
        edge = [0, 1, (1 << lim) - 1, (1 << lim) - 2, 1 << (lim - 1)]
        for d in range(1 << bits):
            edge.append(sum(d << (bits * w) for w in range(64)) & ((1 << lim) - 1))          # every window at d: the carries run end to end
        for w in range(0, lim, bits):
            edge += [(1 << w) - 1, ((1 << (bits - 1)) + 1) << w]
        for k in edge:
            if k < 1 << lim:
                g.add(int_f(k, 5))
        for _ in range(RANDOM_CASES):
            g.add(int_f(rng.randrange(1 << rng.choice((lim, lim, 64, 100))), 5))
    return groups


def _mixed_os_group(rng):
    """xyzzw_add_mixed_os (g1_mul_dev.h): the mixed addition of the G1 iNTT's multiplications.  Unlike xyzzw_add_mixed it has no test for an
    infinite q: its callers only pass table entries, so no such case is asked"""
    q = Q_MOD
    pt = multiple
    g = Group("E_XYZZW_ADD_MIXED_OS", 1)

    def xw(k, var):
        l, i, j, u1, u2 = var
        return xyzz_words(pt(k), l, R261, i, j, u1, u2)

    def aff_top(k):
        """the affine operand at the top of its range (below 1.1 q): canonical + q in the coordinates where that stays below"""
        x, y = pt(k)[0] * R261 % q, pt(k)[1] * R261 % q
        return int_w(x + q if 10 * x < q else x) + int_w(y + q if 10 * y < q else y)
    liftable = [k for k in range(1, 600) if 10 * (pt(k)[0] * R261 % q) < q or 10 * (pt(k)[1] * R261 % q) < q]
    assert len(liftable) >= 16
    ks = [1, 2, 3, 4, 5, 7, 8, 11, 16, 17, 29, 31, 32, 33, 64, 100, 127, 128, 255, 256, 300, 500]
    pair_list = [(1, 2), (2, 1), (3, 5), (7, 11), (16, 17), (127, 128), (255, 300), (500, 1), (5, 5), (1, 1), (33, 33), (256, 256)]
    inf_garbage = int_w(rng.randrange(q)) + int_w(rng.randrange(q)) + int_w(0) + int_w(rng.randrange(q))
    # acc and q distinct, equal (the doubling exit) and opposite (the cancellation exit): every representation of the accumulator contract
    # (x, y up to 5 q above canonical, zz / zzz canonical + q, ZZ != 1), both values of neg_q, and q given as the point or as its opposite
    for ka, kb in pair_list:
        for var in _point_variants(rng):
            for neg in (0, 1):
                g.add(xw(ka, var) + aff_words(pt(kb), R261) + [neg], ec_add(pt(ka), pt(-kb) if neg else pt(kb)))
        for var in _point_variants(rng, full=False):
            for neg in (0, 1):
                g.add(xw(ka, var) + aff_words(pt(-kb), R261) + [neg], ec_add(pt(ka), pt(kb) if neg else pt(-kb)))
    # both operands at the upper ends of their ranges at once
    for kb in liftable[:16]:
        for ka in (kb, -kb, kb + 1):
            for var in _point_variants(rng, full=False):
                for neg in (0, 1):
                    g.add(xw(ka, var) + aff_top(kb) + [neg], ec_add(pt(ka), pt(-kb) if neg else pt(kb)))
    for kb in ks:                                                # acc at infinity: all zero, or ZZ == 0 beside arbitrary coordinates
        for neg in (0, 1):
            want = pt(-kb) if neg else pt(kb)
            g.add([0] * 36 + aff_words(pt(kb), R261) + [neg], want)
            g.add(inf_garbage + aff_words(pt(kb), R261) + [neg], want)
    for _ in range(RANDOM_CASES):
        ka, kb, neg = rng.randrange(1, 512), rng.randrange(1, 512), rng.randrange(2)
        var = (rng.randrange(1, q), rng.randrange(6), rng.randrange(6), False, False)
        g.add(xw(ka, var) + aff_words(pt(kb), R261) + [neg], ec_add(pt(ka), pt(-kb) if neg else pt(kb)))
    return g


def _window_extremes(bits, windows):
    """magnitudes whose signed recoding (glv_digits4 / glv_digits) is the extreme digit in each of the low `windows` windows: +2^(bits-1) throughout
    (every window holds 2^(bits-1), no carry), or -(2^(bits-1) - 1) throughout (the lowest window holds 2^(bits-1) + 1, each later one 2^(bits-1) plus the
    carry of the one below; the last carry is a digit +1 in the window above)"""
    half = 1 << (bits - 1)
    plus = sum(half << (bits * w) for w in range(windows))
    return plus, plus + 1


def mul_scalars(rng):
    """the directed scalars of the G1 multiplications, as [(k, why)].  glv_split is applied INSIDE the functions under test, so a split can only be
    asked for through a scalar that has it; glv_split_model picks those scalars.  What that leaves out of reach, by the definition in glv_dev.h:
    k1 = k - c1 A1 - c2 A2 with c1 <= k B2 / r, c2 <= k B1N / r and A1 B2 + A2 B1N = r, so k1 >= 0 always (neg1 is never set), and k1 = 0 only
    for k = 0; k2 = c1 B1N - c2 B2 lies in (-B1N, B2), so a negative k2 is below 2^64 in magnitude"""
    r = R_MOD
    out = [(k, "small") for k in range(18)]
    out += [(r - 1, "r-1"), (r - 2, "r-2"), ((r - 1) // 2, "(r-1)/2"), (LAMBDA, "lambda"), (LAMBDA + 1, "lambda+1"), (LAMBDA - 1, "lambda-1"),
            (r - LAMBDA, "r-lambda"), (1 << 127, "2^127"), ((1 << 128) + 1, "2^128+1"), ((1 << 128) - 1, "2^128-1")]
    # the halves of the split and the sign of the second one
    assert glv_split_model(0)[:2] == (0, 0)                      # k1 == 0
    k2_zero = [k for k in (1, 17, 1 << 64, (1 << 100) + 12345, GLV_A1 - 1, rng.randrange(1 << 120)) if glv_split_model(k)[1] == 0]
    assert len(k2_zero) >= 5
    out += [(k, "k2 == 0") for k in k2_zero]
    neg2, tries = [], 0
    while len(neg2) < 12:                                        # k2 = -j and k1 between j A1 / B1N and (r - j A2) / B2: inside the domain of the split
        tries += 1
        assert tries < 1000
        j = rng.randrange(1, GLV_B1N) >> rng.choice((0, 0, 20, 60))
        k1 = rng.randrange(j * GLV_A1 // GLV_B1N + 1, (r - j * GLV_A2) // GLV_B2)
        k = (k1 - j * LAMBDA) % r
        if glv_split_model(k) == (k1, j, False, True):
            neg2.append(k)
    out += [(k, "k2 < 0") for k in neg2]
    assert glv_split_model(LAMBDA)[2:] == (False, False)         # k2 > 0 (with k1 > 0: the split of lambda is not (0, 1))
    # every window at its extreme digit, each sign, in both halves at once: as many low windows as keep (k1, k2) inside the domain of the split
    for bits, total, least in ((4, 32, 30), (3, 43, 41)):
        for windows in range(total, 0, -1):
            ext = _window_extremes(bits, windows)
            ks = [(a + b * LAMBDA) % r for a in ext for b in ext]
            if all(glv_split_model(k) == (a, b, False, False) for k, (a, b) in zip(ks, [(a, b) for a in ext for b in ext])):
                break
        assert windows >= least, (bits, windows)
        out += [(k, "extreme digits, %d-bit windows" % bits) for k in ks]
    # what the transform multiplies by: twiddles omega^-j, 1 / n, and their products (the last stage), for every domain size
    for log_n in range(1, MAX_LOG_N + 1):
        n = 1 << log_n
        w_inv, n_inv = pow(omega(log_n), -1, r), pow(n, -1, r)
        out += [(n_inv, "1/n, log_n %d" % log_n), (w_inv, "1/omega, log_n %d" % log_n), (w_inv * n_inv % r, "1/(omega n), log_n %d" % log_n)]
        for j in sorted(set([n // 2 - 1] + [rng.randrange(n // 2) for _ in range(3)]) - {0}):
            out += [(pow(w_inv, j, r) * n_inv % r, "omega^-%d / n, log_n %d" % (j, log_n)), (pow(w_inv, j, r), "omega^-%d, log_n %d" % (j, log_n))]
    assert all(0 <= k < r for k, _ in out)
    return out


def _mul_groups(rng):
    """g1_mul_scalar, g1_mul_scalar_iso, g1_mul_scalar_iso8 (g1_mul_dev.h): the same cases for the three.  A base is m * (1, 2) in some
    representation, so the expected point is (k m mod r) * (1, 2)"""
    q, r = Q_MOD, R_MOD
    cases = []

    def add(m, var, k):
        l, i, j, u1, u2 = var
        cases.append((xyzz_words(g_mul(m), l, R261, i, j, u1, u2) + int_f(k), g_mul(k * m)))

    def top_variant():
        """x, y at 5 q above canonical (the contract says below 6 q) and ZZ, ZZZ at canonical + q (below 1.3 q): the top of what a preceding
        xyzzw_add or xyzzw_double may hand to a later stage"""
        while True:
            l = rng.randrange(2, q)
            if 10 * (l * l % q * R261 % q) < 3 * q and 10 * (l * l * l % q * R261 % q) < 3 * q:
                return (l, 5, 5, True, True)
    AFFINE = (1, 0, 0, False, False)                             # as g1ntt_load leaves a point: canonical x, y, ZZ = ZZZ = 1
    bases = [(1, AFFINE), (2, AFFINE), (rng.randrange(1, r), AFFINE), (rng.randrange(1, r), AFFINE), (r - 1, AFFINE),
             (rng.randrange(1, r), top_variant()), (rng.randrange(1, r), top_variant()), (3, top_variant()),
             (rng.randrange(1, r), (rng.randrange(2, q), 0, 0, False, False)), (rng.randrange(1, r), (rng.randrange(2, q), 5, 0, False, False)),
             (rng.randrange(1, r), (rng.randrange(2, q), 0, 5, False, False))]
    directed = mul_scalars(rng)
    for k, _ in directed:
        for m, var in bases:
            add(m, var, k)
    inf_garbage = int_w(rng.randrange(q)) + int_w(rng.randrange(q)) + int_w(0) + int_w(rng.randrange(q))
    for k, _ in directed[:40] + [(rng.randrange(r), "") for _ in range(24)]:     # the base at infinity
        cases.append(([0] * 36 + int_f(k), None))
        cases.append((inf_garbage + int_f(k), None))
    for n in range(RANDOM_CASES):
        var = AFFINE if n % 2 == 0 else top_variant() if n % 16 == 1 else (rng.randrange(1, q), rng.randrange(6), rng.randrange(6), False, False)
        add(rng.randrange(1, r), var, rng.randrange(r))
    groups = []
    for name in MUL_OPS:
        g = Group(name, 1)
        for words, want in cases:
            g.add(words, want)
        groups.append(g)
    return groups


def generate(device, seed=20260131):
    """all groups of a run: the host-callable primitives, plus the __device__-only ones when `device` (appended: the others are the same either way)"""
    rng = random.Random(seed)
    groups = _field_groups(0, rng) + _field_groups(1, rng) + _scalar_groups(rng)
    groups += _curve_groups(random.Random(seed + 1), device)
    groups.append(_mixed_os_group(random.Random(seed + 2)))
    if device:
        groups += _mul_groups(random.Random(seed + 3))
    return groups


def expected_coverage(device):
    """(name, field) of every primitive a run must hold cases for"""
    return sorted((n, f) for n, v in OPS.items() for f in v[3] if device or not v[4])


# ------------------------------------------------------------------------------------ the program and its files
def write_cases(groups, path):
    with open(path, "wb") as f:
        for g in groups:
            f.write(struct.pack("<5I", g.op, g.field, len(g.cases), g.in_w, g.out_w))
            flat = [w for c in g.cases for w in c]
            f.write(struct.pack("<%dI" % len(flat), *flat))


def read_results(groups, path):
    """-> one list of output word lists per group; the file must hold exactly these groups"""
    data = open(path, "rb").read()
    pos, outs = 0, []
    for g in groups:
        head = struct.unpack_from("<5I", data, pos)
        assert head == (g.op, g.field, len(g.cases), g.in_w, g.out_w), (g.name, head)
        pos += 20
        n = len(g.cases) * g.out_w
        flat = struct.unpack_from("<%dI" % n, data, pos)
        pos += 4 * n
        outs.append([list(flat[k * g.out_w:(k + 1) * g.out_w]) for k in range(len(g.cases))])
    assert pos == len(data), "trailing bytes in the result file"
    return outs


def build_program(outdir):
    """hipcc, as for the other programs of tests/host, but one translation unit per group of primitives, compiled side by side (at most 10 jobs)"""
    src = os.path.join(ROOT, "tests", "host", "arith_kat.hip")
    base = ["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "plonkit_amd", "csrc")]
    jobs = [("main.o", ["-DKAT_MAIN"])] + [("part%d.o" % k, ["-DKAT_PART=%d" % k]) for k in range(KAT_PARTS)]

    def compile_one(job):
        obj = os.path.join(outdir, job[0])
        subprocess.check_call(base + job[1] + ["-c", src, "-o", obj], stderr=subprocess.DEVNULL)
        return obj
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        objs = list(ex.map(compile_one, jobs))
    exe = os.path.join(outdir, "arith_kat")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950"] + objs + ["-o", exe], stderr=subprocess.DEVNULL)
    return exe


def run_program(exe, groups, workdir, host, timeout=600):
    """one process over all groups; -> (results per group, the program's summary line)"""
    tag = "host" if host else "device"
    cases, results = os.path.join(workdir, "cases_%s.bin" % tag), os.path.join(workdir, "results_%s.bin" % tag)
    write_cases(groups, cases)
    r = subprocess.run([exe] + (["--host"] if host else []) + [cases, results], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return read_results(groups, results), r.stdout.strip()
