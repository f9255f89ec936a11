"""Cases and the integer model for the tests of the prover's round kernels (plonkit_amd/csrc/poly.hip) at extreme residues and scan seams.

Python owns the operands and the expected answers.  Every expected value comes from the definition the header gives (include/plonkit_amd.h,
"the polynomial helpers of rounds 2, 4 and 5"), with Python integers, `%`, `pow` and plain loops — never from the oracle library or a port of
the kernels:

    grand product   z_0 = 1,  z_{i+1} = z_i * prod_j (w_j[i] + beta k_j omega^i + gamma) / (w_j[i] + beta sigma_j[i] + gamma),  k = 1, 5, 7, 10
    evaluation      p(z) = sum_i c_i z^i
    division        (p(x) - p(z)) / (x - z) by synthetic division: n coefficients, the top one zero
    coset-major     position k * n + r holds natural index 4 r + k
    gate            q_a a + q_b b + q_c c + q_d d + q_m a b + q_const + q_d_next d[row + 1] + (a on a public-input row) = 0

tests/test_round_cases_host.py holds this model against the oracle's vector operations on random inputs before either judges a kernel.

Elements are canonical Python integers in [0, r).  The device stores an element x as the 256-bit integer x * 2^256 mod r (Montgomery form,
four 64-bit limbs): to_array() / from_array() convert.  The lazy arithmetic of the kernels sees the STORED integer, so the directed vectors are
named by what lies in memory: "stored r - 1" is the element (r - 1) * 2^-256 whose limbs are those of r - 1, the largest a kernel can load.
"""
import random

import numpy as np

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT_R = 1 << 256
R_INV = pow(MONT_R, -1, R_MOD)
NON_RESIDUES = (1, 5, 7, 10)
TWO_ADICITY = 28
ROOT_2_28 = pow(7, (R_MOD - 1) >> TWO_ADICITY, R_MOD)       # the generator of the 2^28 subgroup that bellman's domains use (7 generates Fr*)
SCAN_BLOCK = 2048                                           # poly.h POLY_SCAN_BLOCK: elements per block of the scans and of the evaluation
COSET_GEN = 7


def omega(log_n):
    assert 0 <= log_n <= TWO_ADICITY
    return pow(ROOT_2_28, 1 << (TWO_ADICITY - log_n), R_MOD)


LIMBS_ALL_ONES = (0x30644d << 232) | ((1 << 232) - 1)       # < r: all eight lower 29-bit limbs of the kernels' 9 x 29-bit layer are 2^29 - 1


def stored(s):
    """the element whose stored (Montgomery) integer is s"""
    return s * R_INV % R_MOD


# --------------------------------------------------------------------------- integers <-> device arrays
def _limbs(v):
    return (v & 0xFFFFFFFFFFFFFFFF, (v >> 64) & 0xFFFFFFFFFFFFFFFF, (v >> 128) & 0xFFFFFFFFFFFFFFFF, v >> 192)


def to_array(xs):
    """canonical integers -> uint64 [n, 4], Montgomery form, little-endian limbs"""
    cache = {}
    rows = []
    for x in xs:
        l = cache.get(x)
        if l is None:
            assert 0 <= x < R_MOD
            l = cache[x] = _limbs(x * MONT_R % R_MOD)
        rows.append(l)
    return np.array(rows, dtype=np.uint64).reshape(len(rows), 4)


def to_limbs(x):
    return to_array([x % R_MOD])[0]


def stored_ints(a):
    """uint64 [n, 4] -> the stored integers as they are (a canonical result is < r)"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192) for r in a.tolist()]


def from_array(a):
    """uint64 [n, 4] Montgomery -> canonical integers; refuses a stored integer >= r (the kernels' outputs are canonical residues)"""
    out = []
    for s in stored_ints(a):
        assert s < R_MOD, "not a canonical residue: %x" % s
        out.append(s * R_INV % R_MOD)
    return out


# ------------------------------------------------------------------------------------ the round helpers
def grand_product(w, sigma, beta, gamma, log_n):
    """(z, zero_den): the N values z_0 .. z_{N-1}; zero_den = the lowest row whose denominator vanishes (None if none does; z is None then:
    all N rows count, the last one too — the device inverts the product of all N denominators)"""
    n = 1 << log_n
    assert len(w) == 4 and len(sigma) == 4 and all(len(v) == n for v in list(w) + list(sigma))
    om = omega(log_n)
    k1, k2, k3 = NON_RESIDUES[1:]
    num, den = [1] * n, [1] * n
    bx = beta % R_MOD                                       # beta omega^i
    for i in range(n):
        w0, w1, w2, w3 = w[0][i] + gamma, w[1][i] + gamma, w[2][i] + gamma, w[3][i] + gamma
        num[i] = (w0 + bx) * (w1 + k1 * bx) % R_MOD * ((w2 + k2 * bx) * (w3 + k3 * bx) % R_MOD) % R_MOD
        den[i] = (w0 + beta * sigma[0][i]) * (w1 + beta * sigma[1][i]) % R_MOD * ((w2 + beta * sigma[2][i]) * (w3 + beta * sigma[3][i]) % R_MOD) % R_MOD
        bx = bx * om % R_MOD
    for i in range(n):
        if den[i] == 0:
            return None, i
    # 1 / den_i for all rows from one inversion: pre_i = den_0 .. den_{i-1}, 1 / den_i = pre_i / pre_{i+1}
    pre = [1] * (n + 1)
    for i in range(n):
        pre[i + 1] = pre[i] * den[i] % R_MOD
    inv, back = [0] * n, pow(pre[n], -1, R_MOD)            # back = 1 / pre_{i+1}
    for i in range(n - 1, -1, -1):
        inv[i] = back * pre[i] % R_MOD
        back = back * den[i] % R_MOD
    assert back == 1
    z = [1] * n
    for i in range(n - 1):
        z[i + 1] = z[i] * num[i] % R_MOD * inv[i] % R_MOD
    return z, None


def poly_eval(c, z):
    acc = 0
    for v in reversed(c):
        acc = (acc * z + v) % R_MOD
    return acc


def poly_div_linear(p, z):
    """(p(x) - p(z)) / (x - z): q_{n-1} = 0, q_{k-1} = p_k + z q_k"""
    n = len(p)
    q = [0] * n
    for k in range(n - 1, 0, -1):
        q[k - 1] = (p[k] + z * q[k]) % R_MOD
    return q


def coset_major_index(n):
    """idx with coset_major[k * n + r] = natural[idx[k * n + r]] = natural[4 r + k]"""
    return np.array([4 * r + k for k in range(4) for r in range(n)], dtype=np.int64)


def to_coset_major(nat, n):
    return np.ascontiguousarray(np.asarray(nat)[coset_major_index(n)])


def from_coset_major(cm, n):
    out = np.empty_like(np.asarray(cm))
    out[coset_major_index(n)] = cm
    return out


# ------------------------------------------------------------------------------------- directed vectors
def near_r(n, seed):
    """stored residues within 2^16 of r (the recipe of tests/test_gpu_kernels.py::test_ntt_extreme_residues)"""
    rng = random.Random(seed)
    base = [stored(R_MOD - 1 - rng.randrange(1 << 16)) for _ in range(min(n, 1 << 12))]
    return [base[i % len(base)] for i in range(n)]


def uniform(n, seed):
    """uniform over the whole of [0, r)"""
    rng = random.Random(seed)
    return [rng.randrange(R_MOD) for _ in range(n)]


def directed_vectors(n, seed=1):
    """[(name, n canonical integers)]"""
    top, m1 = stored(R_MOD - 1), R_MOD - 1
    out = [("stored_r_minus_1", [top] * n),
           ("minus_one", [m1] * n),
           ("zero", [0] * n),
           ("one", [1] * n),
           ("stored_r_minus_1_alt_zero_stride_1", [top if i % 2 == 0 else 0 for i in range(n)]),
           ("stored_r_minus_1_alt_zero_stride_%d" % SCAN_BLOCK, [top if (i // SCAN_BLOCK) % 2 == 0 else 0 for i in range(n)]),
           ("near_r", near_r(n, seed)),
           ("stored_limbs_all_ones", [stored(LIMBS_ALL_ONES)] * n)]
    for at in sorted({0, SCAN_BLOCK - 1, SCAN_BLOCK, n - 1}):
        if at < n:
            v = [0] * n
            v[at] = top
            out.append(("single_at_%d" % at, v))
    out.append(("uniform", uniform(n, seed + 1)))
    return out


def directed(n, name, seed=1):
    for k, v in directed_vectors(n, seed):
        if k == name:
            return v
    raise KeyError(name)


def scalar_edges(seed):
    """[(name, value)]: the challenges beta, gamma at their edges; 2^253 is the first value a 253-bit transcript challenge cannot take"""
    rng = random.Random(seed)
    return [("0", 0), ("1", 1), ("r-1", R_MOD - 1), ("r-2", R_MOD - 2), ("2^253", (1 << 253) % R_MOD), ("stored r-1", stored(R_MOD - 1)),
            ("stored limbs all ones", stored(LIMBS_ALL_ONES)), ("random", rng.randrange(R_MOD))]


def eval_points(n, seed):
    """[(name, z)], z != 0: the points of evaluation and division at a polynomial of n coefficients"""
    log_up = max(n - 1, 0).bit_length()                    # the smallest power of two >= n
    rng = random.Random(seed)
    return [("1", 1), ("r-1", R_MOD - 1), ("2", 2), ("1/2", pow(2, -1, R_MOD)), ("omega_n", omega(log_up)), ("omega_2048", omega(11)),
            ("omega_2^28", ROOT_2_28), ("r-2", R_MOD - 2), ("random", rng.randrange(1, R_MOD))]


# -------------------------------------------------------------------------- grand product combinations
PRODUCT_LOG_N = (1, 3, 11, 12, 13)


def grand_product_combinations(log_n):
    """[(name, w[4], sigma[4], beta, gamma)] as listed (before the zero-denominator pruning): the seven wire / sigma patterns crossed with four
    (beta, gamma) pairs — beta = gamma = r - 1; beta = 0 (num = den: z is all ones); gamma = 0 with beta = 1; random — and nine more pairs from
    {0, 1, r - 1, r - 2, 2^253, stored r - 1, stored limbs all ones, random}^2, each on one pattern in turn (the whole cross would take a minute of model time)"""
    n = 1 << log_n
    top_v, zero_v = directed(n, "stored_r_minus_1"), [0] * n
    near = [near_r(n, 10 * log_n + j) for j in range(8)]
    alt = directed(n, "stored_r_minus_1_alt_zero_stride_%d" % SCAN_BLOCK)
    alt_rev = [stored(R_MOD - 1) - v for v in alt]         # the complement: zero where alt is r - 1
    ones_v = directed(n, "stored_limbs_all_ones")
    patterns = [("all stored r-1", [top_v] * 4, [top_v] * 4),
                ("all 0", [zero_v] * 4, [zero_v] * 4),
                ("w stored r-1, sigma 0", [top_v] * 4, [zero_v] * 4),
                ("w 0, sigma stored r-1", [zero_v] * 4, [top_v] * 4),
                ("near r", near[:4], near[4:]),
                ("stride-%d alternation" % SCAN_BLOCK, [alt, alt_rev, alt, alt_rev], [alt_rev, alt, alt_rev, alt]),
                ("all stored limbs 2^29-1", [ones_v] * 4, [ones_v] * 4)]
    e = dict(scalar_edges(100 + log_n))
    core = [("r-1", "r-1"), ("0", "random"), ("1", "0"), ("random", "random")]
    more = [("stored r-1", "stored r-1"), ("r-2", "1"), ("2^253", "r-2"), ("random", "2^253"), ("1", "r-1"), ("r-1", "0"), ("stored limbs all ones", "stored limbs all ones"), ("2^253", "2^253"), ("r-1", "1")]
    out = []
    for pname, w, s in patterns:
        for b, g in core:
            out.append(("%s, beta %s, gamma %s" % (pname, b, g), w, s, e[b], e[g]))
    for k, (b, g) in enumerate(more):
        pname, w, s = patterns[k % len(patterns)]
        out.append(("%s, beta %s, gamma %s" % (pname, b, g), w, s, e[b], e[g]))
    return out


# ------------------------------------------------------------------------------ constant-column circuits
def constant_circuit(log_n, consts, num_inputs, d_next_live, sigma_kind, q_all=R_MOD - 1, seed=0):
    """A width-4 circuit whose wire columns are the constants (a, b, c, d) on every row and whose selectors q_a q_b q_c q_d q_m are q_all (r - 1) on
    every row.  q_d_next is q_all on rows 0 .. N - 2 and 0 on row N - 1 when d_next_live (the gate check has no wrap on the last row), else 0;
    q_const is, row by row, whatever makes the gate equation hold (the + a of the public-input rows included).  sigma_kind: "identity", "column"
    (a seeded shuffle inside each column) or "full" (a seeded shuffle of all 4 N cells: the four constants must be equal) — every cell of a copy
    cycle holds the same value, so each of them is a valid permutation.  Returns a dict of value vectors (canonical integers)."""
    n = 1 << log_n
    a, b, c, d = (v % R_MOD for v in consts)
    m1 = q_all % R_MOD
    assert 0 <= num_inputs < n
    q = [[m1] * n for _ in range(5)]
    q_dn = [m1 if (d_next_live and r < n - 1) else 0 for r in range(n)]
    q_const = [0] * n
    for r in range(n):
        rest = m1 * (a + b + c + d + a * b) + q_dn[r] * d + (a if r < num_inputs else 0)
        q_const[r] = -rest % R_MOD
    cols = [[a] * n, [b] * n, [c] * n, [d] * n]
    for r in range(n):                                      # the gate equation, row by row
        dn = cols[3][r + 1] if r + 1 < n else 0
        pi = cols[0][r] if r < num_inputs else 0
        lhs = (q[0][r] * cols[0][r] + q[1][r] * cols[1][r] + q[2][r] * cols[2][r] + q[3][r] * cols[3][r] + q[4][r] * cols[0][r] * cols[1][r]
               + q_const[r] + q_dn[r] * dn + pi)
        assert lhs % R_MOD == 0, "row %d" % r
    om = omega(log_n)
    dom = [1] * n
    for i in range(1, n):
        dom[i] = dom[i - 1] * om % R_MOD
    rng = random.Random(seed)
    if sigma_kind == "identity":
        target = [(j, i) for j in range(4) for i in range(n)]
    elif sigma_kind == "column":
        target = []
        for j in range(4):
            p = list(range(n))
            rng.shuffle(p)
            target += [(j, i) for i in p]
    elif sigma_kind == "full":
        assert a == b == c == d, "a shuffle across columns needs equal constants"
        target = [(j, i) for j in range(4) for i in range(n)]
        rng.shuffle(target)
    else:
        raise ValueError(sigma_kind)
    assert sorted(target) == [(j, i) for j in range(4) for i in range(n)]
    for cell, (j2, i2) in enumerate(target):                 # copy constraints: a cell and its image hold the same value
        assert cols[cell // n][cell % n] == cols[j2][i2]
    sigma = [[NON_RESIDUES[target[j * n + i][0]] * dom[target[j * n + i][1]] % R_MOD for i in range(n)] for j in range(4)]
    return dict(log_n=log_n, N=n, num_inputs=num_inputs, selectors=q + [q_const, q_dn], sigmas=sigma, columns=cols, inputs=[a] * num_inputs)


M1 = R_MOD - 1
TOP = stored(R_MOD - 1)
# (log_n, (a, b, c, d), public inputs, q_d_next live, sigma[, the selector constant]): 8 is the last count of public inputs on the in-kernel path of the quotient, 9 the
# first on the extended one; every size has cases with inputs and a live q_d_next; (0, 0, 0, 0) commits every wire to the point at infinity
CIRCUIT_CASES = [
    (3, (M1, M1, M1, M1), 3, True, "full"),
    (3, (M1, M1 - 1, 1, 0), 1, True, "column"),
    (3, (M1, M1 - 1, M1 - 2, M1 - 3), 0, False, "column"),
    (3, (0, 0, 0, 0), 0, False, "identity"),
    (3, (0, 0, 0, 0), 1, True, "full"),
    (3, (TOP, TOP, TOP, TOP), 3, True, "full", TOP),
    (11, (M1, M1, M1, M1), 9, True, "full"),
    (11, (M1, M1 - 1, 1, 0), 8, True, "column"),
    (11, (M1, M1 - 1, M1 - 2, M1 - 3), 1, False, "column"),
    (11, (0, 0, 0, 0), 0, False, "identity"),
    (11, (0, 0, 0, 0), 3, True, "full"),
    (11, (TOP, TOP, TOP, TOP), 3, True, "full", TOP),
    (12, (M1, M1, M1, M1), 8, True, "full"),
    (12, (M1, M1 - 1, 1, 0), 9, True, "column"),
    (12, (M1, M1 - 1, M1 - 2, M1 - 3), 3, True, "column"),
    (12, (0, 0, 0, 0), 0, False, "identity"),
    (12, (0, 0, 0, 0), 1, False, "full"),
    # beyond the canonical r - 1 (stored as r - 2^256 mod r, about 0.71 r): columns and selectors whose STORED limbs are those of r - 1
    (12, (TOP, TOP, TOP, TOP), 9, True, "full", TOP),
]


def circuit_id(case):
    log_n, consts, n_in, live, kind = case[:5]
    name = {M1: "r-1", M1 - 1: "r-2", M1 - 2: "r-3", M1 - 3: "r-4", TOP: "stored_r-1"}
    return "2^%d-(%s)-pi%d-%s-%s" % (log_n, ",".join(name.get(v, str(v)) for v in consts), n_in, "dnext" if live else "nodnext", kind)


_CRS = {}


def oracle_setup_and_proof(case):
    """(circuit, Setup, Crs, Proof, debug vectors) of one CIRCUIT_CASES entry through the oracle prover (the crs_42 key, cached by size)"""
    from oracle import oracle_lib as ol, plonk_oracle as po
    c = constant_circuit(*case, seed=sum(case[1]) % 1000 + case[0])           # (a case may end with its selector constant)
    n = c["N"]
    if n not in _CRS:
        _CRS[n] = po.Crs(ol.crs42(n), b"\x00" * 256)
    S = po.setup_from_values([to_array(v) for v in c["selectors"]], [to_array(v) for v in c["sigmas"]], c["num_inputs"])
    P, dbg = po.prove_columns(S, [to_array(v) for v in c["columns"]], c["inputs"], _CRS[n], return_debug=True)
    return c, S, _CRS[n], P, dbg
