"""Cases and the plain model for the copy-constraint checks (plonkit_amd/csrc/copycheck.hip, sigma_decode_dev.h): sigma value -> cell,
is sigma a bijection of the cells, which cell differs from its image.

Everything is Python integers and follows the definitions, not the kernels: a sigma value is decoded by looking it up in the dictionary of the
4N labels k_c * omega^i, bijectivity is a Counter over the images, the first broken copy is found by walking the cells in key order.  For the
domains whose 4N labels do not fit a dictionary (the host program runs every log_n up to 26) decode_value() finds the row from exponentiations
alone and then certifies it with pow(): labels are unique, so an answer that passes k_c * omega^i == x is the answer.

Conventions of include/plonkit_amd.h: a cell is (col, row); packed = col << 30 | row; idx[col * n + row]; key = row * 4 + col ("lowest" is
by key: row first, then a, b, c, d); a refused value gives 0xFFFFFFFF.  A sigma value here is a canonical integer below r, or Raw(v): the
256-bit integer v >= r as it would sit in memory, which is no field element at all.

The variable tables, successors(), index_of() and sigmas_of() come from tests/gen/perm_cases.py, which this module imports and leaves alone.
"""
import collections
import random

from tests.gen import perm_cases as pc
from tests.gen.perm_cases import R_MOD, NON_RESIDUES, omega

NOT_A_LABEL = 0xFFFFFFFF
MONT_R = (1 << 256) % R_MOD
OK, KIND_NOT_A_LABEL, KIND_NOT_BIJECTIVE, KIND_BROKEN = 0, 1, 2, 3


class Raw(int):
    """limbs as stored, >= r: a non-canonical residue"""


def key(col, row):
    return 4 * row + col


def cell_of_key(k):
    return (k & 3, k >> 2)


def pack(col, row):
    return (col << 30) | row


def unpack(p):
    return (p >> 30, p & 0x3FFFFFFF)


# ------------------------------------------------------------------------------------------------ the model
_LABELS = {}


def labels(log_n):
    """{k_c * omega^i: c << 30 | i} over the 4N cells"""
    d = _LABELS.get(log_n)
    if d is None:
        d, w, x = {}, omega(log_n), 1
        for i in range(1 << log_n):
            for c in range(4):
                d[NON_RESIDUES[c] * x % R_MOD] = pack(c, i)
            x = x * w % R_MOD
        assert len(d) == 4 << log_n                                         # the four cosets are disjoint
        _LABELS[log_n] = d
    return d


def decode(sig, log_n):
    """four columns of sigma values -> (idx, bad_key): idx[col * n + row], NOT_A_LABEL where refused; bad_key = the lowest refused key or None"""
    n, lab = 1 << log_n, labels(log_n)
    idx, bad = [NOT_A_LABEL] * (4 * n), None
    for col in range(4):
        assert len(sig[col]) == n
        for row, x in enumerate(sig[col]):
            p = NOT_A_LABEL if isinstance(x, Raw) else lab.get(x, NOT_A_LABEL)
            idx[col * n + row] = p
            if p == NOT_A_LABEL and (bad is None or key(col, row) < bad):
                bad = key(col, row)
    return idx, bad


def decode_value(x, log_n):
    """one value by exponentiation, for any log_n: the packed cell or NOT_A_LABEL.  x is a label of coset c iff (x / k_c)^N = 1; its row is
    then read off bit by bit from the powers (x / k_c * omega^-(bits so far))^(N / 2^(t+1)) = +-1, and the result is certified by pow()."""
    if isinstance(x, Raw):
        assert x >= R_MOD
        return NOT_A_LABEL
    assert 0 <= x < R_MOD
    n, w = 1 << log_n, omega(log_n)
    for c in range(4):
        y = x * pow(NON_RESIDUES[c], -1, R_MOD) % R_MOD
        if y == 0 or pow(y, n, R_MOD) != 1:
            continue
        i, w_inv = 0, pow(w, -1, R_MOD)
        for t in range(log_n):
            if pow(y * pow(w_inv, i, R_MOD) % R_MOD, n >> (t + 1), R_MOD) != 1:
                i |= 1 << t
        assert NON_RESIDUES[c] * pow(w, i, R_MOD) % R_MOD == x              # the certificate
        return pack(c, i)
    return NOT_A_LABEL


def imageless(idx):
    """the lowest key of a cell that is the image of no cell, None if every cell is one.  (Call it on an idx without refusals.)"""
    n = len(idx) // 4
    seen = collections.Counter(p for p in idx if p != NOT_A_LABEL)
    for k in range(4 * n):
        col, row = cell_of_key(k)
        if seen[pack(col, row)] == 0:
            return k
    return None


def first_broken(idx, values):
    """values: four columns already extended to n.  The lowest key of a cell whose value differs from its image's, with that image"""
    n = len(idx) // 4
    for k in range(4 * n):
        col, row = cell_of_key(k)
        c2, r2 = unpack(idx[col * n + row])
        if values[col][row] != values[c2][r2]:
            return (col, row), (c2, r2)
    return None


def extend(cols, n):
    return [list(c) + [0] * (n - len(c)) for c in cols]


def report(sig, log_n, columns=None):
    """(kind, cell, image) as plk_setup_check_permutation (columns None) / plk_check_copies report it: refusals first, then bijectivity,
    then the copies"""
    idx, bad = decode(sig, log_n)
    if bad is not None:
        return (KIND_NOT_A_LABEL, cell_of_key(bad), None)
    k = imageless(idx)
    if k is not None:
        return (KIND_NOT_BIJECTIVE, cell_of_key(k), None)
    if columns is not None:
        hit = first_broken(idx, extend(columns, 1 << log_n))
        if hit:
            return (KIND_BROKEN, hit[0], hit[1])
    return (OK, None, None)


# ------------------------------------------------------------------------------------- values that are no label
def non_labels(log_n, rng):
    """[(name, value)]: what the decode must refuse at this domain, each checked against the model's exponentiation"""
    w = omega(log_n)
    i = rng.randrange(1 << log_n)
    some_label = NON_RESIDUES[rng.randrange(4)] * pow(w, rng.randrange(1 << log_n), R_MOD) % R_MOD
    out = [("zero", 0), ("2 * omega^%d" % i, 2 * pow(w, i, R_MOD) % R_MOD), ("omega_2N", omega(log_n + 1)),
           ("r - 1", R_MOD - 1), ("r, not canonical", Raw(R_MOD)), ("a label + r, not canonical", Raw(some_label * MONT_R % R_MOD + R_MOD))]
    out = [(name, v) for name, v in out if decode_value(v, log_n) == NOT_A_LABEL]       # r - 1 = omega^(N/2) is a label of every domain
    assert {name for name, _ in out} >= {"zero", "omega_2N", "r, not canonical"} and any(name.startswith("2 *") for name, _ in out)
    return out


def label_rows(log_n, rng):
    n = 1 << log_n
    return sorted({0, 1 % n, n // 2, n - 1} | {rng.randrange(n) for _ in range(3)})


def stored_int(x):
    """the 256-bit integer the library sees for a value: Montgomery form of a canonical integer, a Raw as it is"""
    return int(x) if isinstance(x, Raw) else x * MONT_R % R_MOD


def to_array(xs):
    """values -> uint64 [n, 4], little-endian limbs"""
    import numpy as np
    return np.array([[(stored_int(x) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for x in xs], dtype=np.uint64).reshape(len(xs), 4)


# ---------------------------------------------------------------------------------------------------- cases
DIRECT_LOG_N = (1, 2, 3, 6, 8, 11)            # 6: one wave per column; 8: 4 blocks of 256 cells
LARGE_LOG_N = 16


def table(log_n, seed=None):
    """a variable table of a size/log_n case of perm_cases.py: four columns of ids, a quarter as many distinct ids as cells, one in eight
    the dummy"""
    rng = random.Random(5000 + log_n if seed is None else seed)
    n4 = 4 << log_n
    num_vars = max(4, n4)
    pool = sorted({num_vars - 1} | {rng.randrange(1, num_vars) for _ in range(max(2, n4 // 4))})
    ids = [0 if rng.randrange(8) == 0 else pool[rng.randrange(len(pool))] for _ in range(n4)]
    return pc.Case("copy/log_n=%d" % log_n, log_n, num_vars, [ids[c::4] for c in range(4)])


def perm_case_names():
    """the cases of perm_cases.py up to the 2^12 domain (pass counts, sizes, hubs, all dummy, no dummy, all distinct) and the single cycle
    over all cells, which lives at 2^14"""
    return tuple(name for name in pc.CASE_NAMES if name == "hub/one_id_everywhere" or pc.case(name).log_n <= 12)


_DECODE_CASES = {}


def decode_cases():
    """{name: (log_n, sigma columns, expected idx)} with valid sigmas: the direct tables and perm_cases.py's cases up to 2^12"""
    if not _DECODE_CASES:
        for log_n in DIRECT_LOG_N:
            c = table(log_n)
            _DECODE_CASES[c.name] = (log_n, pc.sigmas_of(c.nxt, log_n), pc.index_of(c.nxt))
        for name in perm_case_names():
            c = pc.case(name)
            _DECODE_CASES[name] = (c.log_n, pc.sigmas_of(c.nxt, c.log_n), pc.index_of(c.nxt))
    return _DECODE_CASES


REFUSAL_LOG_N = 8


def refusal_cells():
    """where a non-label is planted at the 2^8 domain (one lane per cell, one block of 256 lanes per column): (a, 0), (d, N - 1), the last
    lane of a block and the first lane of the next (b[255] | c[0]), the two sides of a wave's seam (b[63] | b[64]), and two cells at once,
    the lower key once in the higher column"""
    n = 1 << REFUSAL_LOG_N
    return [[(0, 0)], [(3, n - 1)], [(1, n - 1)], [(2, 0)], [(1, 63)], [(1, 64)], [(2, 200), (1, 77)], [(3, 5), (0, 6)]]


_REFUSAL_CASES = []


def refusal_cases():
    """[(name, log_n, sigma columns with planted non-labels, the planted cells)]"""
    if not _REFUSAL_CASES:
        rng = random.Random(61)
        c = table(REFUSAL_LOG_N)
        base = pc.sigmas_of(c.nxt, REFUSAL_LOG_N)
        for what, v in non_labels(REFUSAL_LOG_N, rng):
            for cells in refusal_cells():
                sig = [list(col) for col in base]
                for col, row in cells:
                    sig[col][row] = v
                _REFUSAL_CASES.append(("%s at %s" % (what, cells), REFUSAL_LOG_N, sig, cells))
    return _REFUSAL_CASES


def shared_image_case(log_n):
    """a valid sigma in which one cell's value is overwritten by another cell's: two cells share an image, so some cell is nobody's"""
    rng = random.Random(70 + log_n)
    c = table(log_n)
    sig = pc.sigmas_of(c.nxt, log_n)
    n = 1 << log_n
    while True:
        (c1, r1), (c2, r2) = [(rng.randrange(4), rng.randrange(n)) for _ in range(2)]
        if sig[c1][r1] != sig[c2][r2]:
            break
    sig[c1][r1] = sig[c2][r2]
    return sig


# -- the hand-built N = 8 circuit of the assembled tests, written out again: one public input x; rows: 0 public input (q_a = -1); 1 x * y = xy
#    (q_m = 1, q_c = -1); 2 xy + y = s (q_a = q_b = 1, q_c = -1); 3 a = s with all selectors zero; 4..7 empty.  Copy cycles: x (0a, 1a),
#    y (1b, 2b), xy (1c, 2a), s (2c, 3a).
HAND_LOG_N = 3


def hand_built():
    """-> (q: 7 selector columns, sig: 4 sigma columns, cols: 4 value columns), canonical integers, N = 8"""
    n, x, y = 1 << HAND_LOG_N, 3, 11
    xy, s, m1 = x * y % R_MOD, (x * y + y) % R_MOD, R_MOD - 1
    q = [[0] * n for _ in range(7)]                                         # q_a q_b q_c q_d q_m q_const q_d_next
    q[0][0] = m1
    q[4][1], q[2][1] = 1, m1
    q[0][2], q[1][2], q[2][2] = 1, 1, m1
    cols = [[0] * n for _ in range(4)]
    cols[0][:4] = [x, x, xy, s]
    cols[1][1:3] = [y, y]
    cols[2][1:3] = [xy, s]
    nxt = list(range(4 * n))
    for (c1, r1), (c2, r2) in (((0, 0), (0, 1)), ((1, 1), (1, 2)), ((2, 1), (0, 2)), ((2, 2), (0, 3))):
        nxt[key(c1, r1)], nxt[key(c2, r2)] = key(c2, r2), key(c1, r1)
    return q, pc.sigmas_of(nxt, HAND_LOG_N), cols


def three_cycle():
    """N = 8, no gates: one cycle a[1] -> c[4] -> b[6] -> a[1] holding (v, v, w).  Two cells differ from their image (c[4] from b[6], b[6]
    from a[1]); the lowest by key is c[4] (row 4), not b[6]"""
    n = 1 << HAND_LOG_N
    nxt = list(range(4 * n))
    cyc = [key(0, 1), key(2, 4), key(1, 6)]
    for k in range(3):
        nxt[cyc[k]] = cyc[(k + 1) % 3]
    cols = [[0] * n for _ in range(4)]
    cols[0][1], cols[2][4], cols[1][6] = 77, 77, 78
    return pc.sigmas_of(nxt, HAND_LOG_N), cols


def beyond_rows():
    """N = 8, rows = 3: a[1] = 5 is tied to d[6], a cell of the zero extension"""
    n = 1 << HAND_LOG_N
    nxt = list(range(4 * n))
    nxt[key(0, 1)], nxt[key(3, 6)] = key(3, 6), key(0, 1)
    cols = [[0] * 3 for _ in range(4)]
    cols[0][1] = 5
    return pc.sigmas_of(nxt, HAND_LOG_N), cols


# ------------------------------------------------------------------------------------------- wrong decoders
# What a wrong kernel would return for one value; tests/test_copy_cases_host.py asserts that the cases tell each from decode().
def _right(x, log_n):
    return NOT_A_LABEL if isinstance(x, Raw) else labels(log_n).get(x, NOT_A_LABEL)


def wrong_ignores_coset(x, log_n):
    p = _right(x, log_n)
    return p if p == NOT_A_LABEL else pack(0, unpack(p)[1])


def wrong_bits_reversed(x, log_n):
    p = _right(x, log_n)
    if p == NOT_A_LABEL:
        return p
    col, row = unpack(p)
    return pack(col, int(format(row, "0%db" % log_n)[::-1], 2))


def wrong_last_row(x, log_n):
    """the loop over the bits stops one short when every bit is set: row N - 1 comes back as N / 2 - 1"""
    p = _right(x, log_n)
    if p == NOT_A_LABEL:
        return p
    col, row = unpack(p)
    return pack(col, row & ~(1 << (log_n - 1))) if row == (1 << log_n) - 1 else p


def wrong_accepts_order_2n(x, log_n):
    """no acceptance rule: a value of <omega_2N> comes back as the cell of its square root's floor"""
    p = _right(x, log_n)
    if p != NOT_A_LABEL or isinstance(x, Raw):
        return p
    p2 = labels(log_n + 1).get(x, NOT_A_LABEL)
    if p2 == NOT_A_LABEL:
        return p2
    col, row = unpack(p2)
    return pack(col, row >> 1)


WRONG_DECODERS = (wrong_ignores_coset, wrong_bits_reversed, wrong_last_row, wrong_accepts_order_2n)


def decode_with(fn, sig, log_n):
    n = 1 << log_n
    return [fn(sig[col][row], log_n) for col in range(4) for row in range(n)]
