"""Cases and the model for the tests of the setup's copy-constraint permutation (plonkit_amd/csrc/perm.hip, k_sigma_from_index in poly.hip).

The rule is the one stated at the top of perm.hip and in SURVEY.md A.3: the occurrences of a variable id, taken in row-major order (gate by
gate, a to d inside a gate), map each to the NEXT one and the last to the first; the dummy id 0 and an id that occurs once keep the identity.
successors() states it with a dict of lists: no sort, no numpy, nothing of the kernels.  tests/test_perm_cases_host.py holds it against the
oracle's two setups before it judges a kernel, and shows on the CPU that the cases below tell a wrong sort or a wrong link from the right one.

A position is p = 4 * row + col.  The device answers in two forms (include/plonkit_amd.h, plk_setup_permutation_dev):
    index   idx[col * n + row] = col' << 30 | row'            (col', row') = the successor of (col, row)
    sigma   sigma_col[row]     = k_col' * omega_n^row'        k = 1, 5, 7, 10

successors_vectorised() is a second form of the same rule (one stable argsort) for the single 2^24 case, where the dict would take minutes;
the first form holds it on every small case (tests/test_perm_cases_host.py).

What the shapes reach, in the kernels' terms: the sort works on the 4n pairs in tiles of 4096, one wave per tile walking 64 positions per step;
it runs ceil(bits(num_vars - 1) / 8) passes of 8 bits; the (digit, tile) table of a pass is scanned in blocks of 2048 words, i.e. 8 tiles.
"""
import random

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NON_RESIDUES = (1, 5, 7, 10)
ROOT_2_28 = pow(7, (R_MOD - 1) >> 28, R_MOD)
TILE, WAVE = 4096, 64


def omega(log_n):
    return pow(ROOT_2_28, 1 << (28 - log_n), R_MOD)


def passes(num_vars):
    """8-bit passes the sort takes for ids below num_vars"""
    bits = 1
    while bits < 32 and (1 << bits) < num_vars:
        bits += 1
    return (bits + 7) // 8


# ------------------------------------------------------------------------------------------------ the model
def successors(cols):
    """cols: four lists of n ids -> nxt[p] for every position p = 4 * row + col"""
    n = len(cols[0])
    occ = {}
    for row in range(n):
        for col in range(4):
            v = cols[col][row]
            if v != 0:
                occ.setdefault(v, []).append(4 * row + col)
    nxt = list(range(4 * n))
    for lst in occ.values():
        for k, p in enumerate(lst):
            nxt[p] = lst[(k + 1) % len(lst)]
    return nxt


def index_of(nxt):
    """the packed index: idx[col * n + row] = col' << 30 | row'"""
    n = len(nxt) // 4
    idx = [0] * (4 * n)
    for p, q in enumerate(nxt):
        idx[(p & 3) * n + (p >> 2)] = ((q & 3) << 30) | (q >> 2)
    return idx


def sigmas_of(nxt, log_n):
    """the four sigma columns as canonical integers: sigma_col[row] = k_col' * omega^row'"""
    n = 1 << log_n
    assert len(nxt) == 4 * n
    w, dom = omega(log_n), [1] * n
    for i in range(1, n):
        dom[i] = dom[i - 1] * w % R_MOD
    sig = [[0] * n for _ in range(4)]
    for p, q in enumerate(nxt):
        sig[p & 3][p >> 2] = NON_RESIDUES[q & 3] * dom[q >> 2] % R_MOD
    return sig


def successors_vectorised(V):
    """the same rule for a uint32 [4, n] table, by one stable argsort of the 4n ids in row-major order -> int64 [4n]"""
    import numpy as np
    n4 = V.shape[1] * 4
    flat = np.ascontiguousarray(V.T).reshape(-1)
    order = np.argsort(flat, kind="stable")
    sv = flat[order]
    first = np.empty(n4, dtype=bool)
    first[0] = True
    np.not_equal(sv[1:], sv[:-1], out=first[1:])
    start = np.maximum.accumulate(np.where(first, np.arange(n4, dtype=np.int64), 0))      # sorted index of the first occurrence of each id
    last = np.empty(n4, dtype=bool)
    last[-1] = True
    last[:-1] = first[1:]
    succ = np.where(last, order[start], np.roll(order, -1))
    succ = np.where(sv == 0, order, succ)
    nxt = np.empty(n4, dtype=np.int64)
    nxt[order] = succ
    return nxt


def index_of_vectorised(nxt):
    import numpy as np
    n = nxt.shape[0] // 4
    packed = (((nxt & 3) << 30) | (nxt >> 2)).astype(np.uint32)
    return np.ascontiguousarray(packed.reshape(n, 4).T).reshape(-1)


# ---------------------------------------------------------------------------------------------- wrong models
# What a wrong kernel would compute; tests/test_perm_cases_host.py asserts that the cases tell each from successors().  (These may sort:
# they are not the reference.)
def wrong_truncated_sort(cols, bits):
    """a sort that looks at the low `bits` bits of the key only (its last passes skipped), followed by the linking rule of k_perm_next as it
    is written: the next sorted entry if it holds the same id, else the lower bound of the id found by bisection"""
    n = len(cols[0])
    mask = (1 << bits) - 1
    pairs = sorted(((cols[p & 3][p >> 2], p) for p in range(4 * n)), key=lambda kp: kp[0] & mask)      # stable
    nxt = list(range(4 * n))
    for i, (v, p) in enumerate(pairs):
        if v == 0:
            continue
        if i + 1 < 4 * n and pairs[i + 1][0] == v:
            nxt[p] = pairs[i + 1][1]
        else:
            lo, hi = 0, i
            while lo < hi:
                mid = (lo + hi) >> 1
                if pairs[mid][0] < v:
                    lo = mid + 1
                else:
                    hi = mid
            nxt[p] = pairs[lo][1]
    return nxt


def _occurrences(cols, with_dummy=False):
    occ = {}
    for row in range(len(cols[0])):
        for col in range(4):
            v = cols[col][row]
            if v != 0 or with_dummy:
                occ.setdefault(v, []).append(4 * row + col)
    return occ


def wrong_reversed(cols):
    """an unstable order inside a cycle: every occurrence maps to the previous one"""
    nxt = list(range(4 * len(cols[0])))
    for lst in _occurrences(cols).values():
        for k, p in enumerate(lst):
            nxt[p] = lst[k - 1]
    return nxt


def wrong_no_wrap(cols):
    """the last occurrence keeps the identity"""
    nxt = list(range(4 * len(cols[0])))
    for lst in _occurrences(cols).values():
        for k, p in enumerate(lst[:-1]):
            nxt[p] = lst[k + 1]
    return nxt


def wrong_dummy_linked(cols):
    """id 0 linked like any other"""
    nxt = list(range(4 * len(cols[0])))
    for lst in _occurrences(cols, with_dummy=True).values():
        for k, p in enumerate(lst):
            nxt[p] = lst[(k + 1) % len(lst)]
    return nxt


def wrong_tile_local_wrap(cols):
    """the last occurrence wraps to the first one inside its own 4096-entry tile of the sorted array, not to the global first"""
    occ = _occurrences(cols, with_dummy=True)
    nxt = list(range(4 * len(cols[0])))
    start = 0
    for v in sorted(occ):
        lst = occ[v]
        if v != 0:
            for k, p in enumerate(lst[:-1]):
                nxt[p] = lst[k + 1]
            last = start + len(lst) - 1
            nxt[lst[-1]] = lst[max(start, last // TILE * TILE) - start]
        start += len(lst)
    return nxt


# ---------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, log_n, num_vars, cols):
        n = 1 << log_n
        assert len(cols) == 4 and all(len(c) == n for c in cols), name
        assert all(0 <= v < num_vars for c in cols for v in c), name            # the entry point's precondition
        self.name, self.log_n, self.num_vars, self.cols = name, log_n, num_vars, cols
        self._nxt = None

    @property
    def nxt(self):
        if self._nxt is None:                                                   # computed once, shared by the tests of a session
            self._nxt = successors(self.cols)
        return self._nxt


def _from_positions(ids):
    """a list of 4n ids in position order (p = 4 * row + col) -> four columns"""
    return [ids[c::4] for c in range(4)]


def _draw(rng, n4, pool, zero_share=8):
    """n4 ids drawn from the pool, one in `zero_share` the dummy (0: none)"""
    return [0 if zero_share and rng.randrange(zero_share) == 0 else pool[rng.randrange(len(pool))] for _ in range(n4)]


def _pool(rng, size, num_vars):
    """`size` distinct non-zero ids below num_vars, the largest one among them"""
    got = {num_vars - 1}
    while len(got) < size:
        got.add(rng.randrange(1, num_vars))
    return sorted(got)


THREE_PASS = 1 << 21                      # the variable count of the 2^20-gate circuits: 21-bit ids


def pass_ids(num_vars):
    """the ids of a pass-count case: low parts that differ in the lowest digit only and in a middle digit only, each under several values of
    the top digit of this pass count (so: pairs that differ ONLY there), kept where they are below num_vars; the largest id is among them"""
    P = passes(num_vars)
    shift = 8 * (P - 1)
    lows = {0, 1, 2, 0x7f, 0xff}
    for mid in range(1, P - 1):
        lows |= {1 << (8 * mid), (1 << (8 * mid)) | 1, (0xff << (8 * mid)) | 1, (0x80 << (8 * mid))}
    lows |= {(1 << shift) - 1} if shift else set()
    top = (num_vars - 1) >> shift
    ids = set()
    for hi in {0, 1, 2, 0x80, 0xff, top} if shift else {0}:
        for low in lows:
            v = (hi << shift) | low
            if 0 < v < num_vars:
                ids.add(v)
    if num_vars <= 256:
        ids = set(range(1, num_vars))
    ids.add(num_vars - 1)
    return sorted(ids)


PASS_NUM_VARS = (2, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1, 1 << 32)
SIZE_LOG_N = (1, 2, 3, 4, 10, 11, 12, 13, 14)


def _build_passes(num_vars):
    rng = random.Random(1000 + num_vars % 9973)
    return Case("passes/num_vars=%d" % num_vars, 10, num_vars, _from_positions(_draw(rng, 4096, pass_ids(num_vars), zero_share=4)))


def _build_size(log_n):
    rng = random.Random(2000 + log_n)
    n4 = 4 << log_n
    return Case("size/log_n=%d" % log_n, log_n, THREE_PASS, _from_positions(_draw(rng, n4, _pool(rng, max(2, n4 // 4), THREE_PASS))))


def _build_hub_ab():
    """one id on every row of columns a and b: 32768 occurrences over all 16 tiles, a cycle across every tile seam and a wrap across tiles"""
    rng = random.Random(3001)
    n = 1 << 14
    rest = _draw(rng, 2 * n, _pool(rng, n // 2, THREE_PASS))
    return Case("hub/a_and_b_columns", 14, THREE_PASS, [[0x12345] * n, [0x12345] * n, rest[:n], rest[n:]])


def _build_wave_64_65():
    """one id on the 64 positions of a wave step, another on 65 (a step and the first lane of the next), at a tile seam too (log_n = 11): in
    the first pass all 64 lanes of a step hold one digit"""
    rng = random.Random(3002)
    ids = _draw(rng, 8192, _pool(rng, 2048, THREE_PASS))
    ids[5 * WAVE:6 * WAVE] = [0x0a0b0c] * 64
    ids[9 * WAVE:10 * WAVE + 1] = [0x0a0b0d] * 65
    ids[TILE - WAVE:TILE] = [0x1f0001] * 64                    # the last step of tile 0
    ids[TILE:TILE + WAVE + 1] = [0x1f0002] * 65                # the first step of tile 1 and one lane more
    return Case("hub/wave_of_64_and_65", 11, THREE_PASS, _from_positions(ids))


def _build_alternating():
    """two ids alternating position by position over two tiles.  They differ in the top digit only: in the first two passes every lane of
    every step holds one digit (64 equal lanes, 4096 per tile), the last pass ranks 32 lanes of each digit per step and pulls the two apart"""
    return Case("hub/two_ids_alternating", 11, THREE_PASS, _from_positions([0x012345, 0x112345] * 4096))


def _build_distinct_digits():
    """wave steps whose 64 lanes hold 64 distinct lowest digits (every id twice: two such steps, the second in reverse order), and two whose
    lanes hold 64 distinct middle digits under one lowest digit (they stay together through the first pass)"""
    rng = random.Random(3004)
    ids = _draw(rng, 4096, _pool(rng, 1024, THREE_PASS))
    low = [0x030000 | (4 * k + 1) for k in range(64)]
    mid = [0x050007 | ((4 * k + 2) << 8) for k in range(64)]
    rng.shuffle(mid)
    ids[3 * WAVE:4 * WAVE] = low
    ids[40 * WAVE:41 * WAVE] = low[::-1]
    ids[7 * WAVE:8 * WAVE] = mid
    ids[50 * WAVE:51 * WAVE] = mid
    return Case("hub/64_distinct_digits", 10, THREE_PASS, _from_positions(ids))


def _build_single_cycle():
    """one non-zero id everywhere: a single cycle in which position p goes to p + 1 mod 4n"""
    return Case("hub/one_id_everywhere", 14, THREE_PASS, [[0x1abcde] * (1 << 14) for _ in range(4)])


def _build_all_dummy():
    return Case("degenerate/all_dummy", 12, THREE_PASS, [[0] * 4096 for _ in range(4)])


def _build_no_dummy():
    """no id 0: the smallest id's group starts at sorted index 0, where the lower-bound search of its wrap ends"""
    rng = random.Random(4002)
    return Case("degenerate/no_dummy", 12, THREE_PASS, _from_positions(_draw(rng, 1 << 14, _pool(rng, 3000, THREE_PASS), zero_share=0)))


def _build_all_distinct():
    rng = random.Random(4003)
    return Case("degenerate/all_distinct", 12, THREE_PASS, _from_positions(rng.sample(range(1, THREE_PASS), 1 << 14)))


def _build_largest_last():
    """the largest id at the very last position (and at three earlier ones): its last occurrence is the last sorted entry, which has no
    neighbour to compare with"""
    rng = random.Random(4004)
    ids = _draw(rng, 1 << 14, _pool(rng, 3000, THREE_PASS - 1))
    for p in (17, 4096, 9999, (1 << 14) - 1):
        ids[p] = THREE_PASS - 1
    assert max(ids) == THREE_PASS - 1 and ids[-1] == THREE_PASS - 1
    return Case("degenerate/largest_id_last", 12, THREE_PASS, _from_positions(ids))


_BUILDERS = {}
for _m in PASS_NUM_VARS:
    _BUILDERS["passes/num_vars=%d" % _m] = (_build_passes, _m)
for _l in SIZE_LOG_N:
    _BUILDERS["size/log_n=%d" % _l] = (_build_size, _l)
for _name, _fn in (("hub/a_and_b_columns", _build_hub_ab), ("hub/wave_of_64_and_65", _build_wave_64_65), ("hub/two_ids_alternating", _build_alternating),
                   ("hub/64_distinct_digits", _build_distinct_digits), ("hub/one_id_everywhere", _build_single_cycle),
                   ("degenerate/all_dummy", _build_all_dummy), ("degenerate/no_dummy", _build_no_dummy),
                   ("degenerate/all_distinct", _build_all_distinct), ("degenerate/largest_id_last", _build_largest_last)):
    _BUILDERS[_name] = (_fn,)
CASE_NAMES = tuple(_BUILDERS)
BOTH_OUTPUTS = ("passes/num_vars=4294967296", "size/log_n=14", "hub/a_and_b_columns")     # asked for index and sigmas in one call
_CACHE = {}


def case(name):
    """the case of that name, built once per process"""
    c = _CACHE.get(name)
    if c is None:
        b = _BUILDERS[name]
        c = _CACHE[name] = b[0](*b[1:])
        assert c.name == name
    return c


# ------------------------------------------------------------------------------------- the one large case
LARGE_LOG_N, LARGE_NUM_VARS, LARGE_HUB = 24, 1 << 26, 0x2a5a5a5


def large_case():
    """uint32 [4, 2^24]: ids up to 2^26 (four passes), a pool of 2^24 ids so that most occur a few times, one hub over the whole of column b,
    the largest id present.  4n = 2^26 positions are 16384 tiles: 2048 block totals, two per thread of the top-level scan."""
    import numpy as np
    rng = np.random.default_rng(24)
    n = 1 << LARGE_LOG_N
    pool = rng.integers(1, LARGE_NUM_VARS, size=n, dtype=np.uint32)
    V = pool[rng.integers(0, n, size=(4, n))]
    V[rng.integers(0, 8, size=(4, n)) == 0] = 0
    V[1] = LARGE_HUB
    V[3, -1] = V[0, 5] = V[2, n // 2] = LARGE_NUM_VARS - 1
    return np.ascontiguousarray(V)
