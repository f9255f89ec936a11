"""Python-integer model of the multi-point openings FROM VALUES ON THE DOMAIN (plonkit_amd/csrc/kzg_multi_values.hip,
kzg_multi_values_plan.h), step by step as the kernels and the host take them, for N = 2^log_n <= 32.

Plain modular arithmetic on canonical residues, no numpy, no oracle.  Polynomials enter as their N values f[x] = f(omega^x).
  1. P_x = prod_j (omega^x - t_j) with a vanishing factor replaced by 1, ONE inversion of prod_x P_x, prefix and suffix products,
     1 / d_xj = (1 / P_x) prod_{l != j} d_xl
  2. S_ij = sum_{x != k_j} f_i[x] omega^x / d_xj; y_ij = -(t_j^N - 1) / N * S_ij off the domain, f_i[k_j] on it
  3. h[x] = sum_j (G_j[x] - g_j) / d_xj, at x = k_j term j is -(sum_i m_ij S_ij - g_j (N - 1) / 2) / t_j
  4. the same operator at u over the polynomials and h, the value at u taken from sum_i c_i r_i(u)
The definition (interpolate, long-divide: tests/gen/kzg_multi_cases.py) is the referee, reached through the integer NTT below.
WRONG names four plausible mistakes; the host test shows that each fails on at least one case."""
from tests.gen import kzg_multi_cases as km

R = km.R
WRONG = ("vanishing_factor_zero", "ordinary_at_k", "g_without_weights", "value_at_u_zero")


def inv(a):
    """1 / a, and 0 for 0 as the library's host inversion has it"""
    return pow(a, -1, R) if a % R else 0


def ntt(a, log_n, inverse=False):
    """values a(omega^x) from coefficients (radix 2, recursive), or back"""
    n = 1 << log_n
    assert len(a) == n
    w = km.omega(log_n) if log_n else 1
    if inverse:
        w = inv(w)

    def rec(v, root):
        if len(v) == 1:
            return list(v)
        even, odd = rec(v[0::2], root * root % R), rec(v[1::2], root * root % R)
        half, out, t = len(v) // 2, [0] * len(v), 1
        for k in range(half):
            out[k] = (even[k] + t * odd[k]) % R
            out[k + half] = (even[k] - t * odd[k]) % R
            t = t * root % R
        return out

    out = rec([x % R for x in a], w)
    return [x * inv(n) % R for x in out] if inverse else out


def domain(log_n):
    w = km.omega(log_n)
    return [pow(w, x, R) for x in range(1 << log_n)]


def on_domain(t, log_n):
    return pow(t, 1 << log_n, R) == 1


def eval_scale(t, log_n):
    n = 1 << log_n
    return (-(pow(t, n, R) - 1) * inv(n)) % R


def rest_sum(log_n):
    return ((1 << log_n) - 1) * inv(2) % R


# ---------------------------------------------------------------------------------------------- step 1
def inverses(log_n, points, wrong=None):
    """(inv[x][j] = 1 / d_xj with 1 where d vanishes, ks[j] = k_j or None) through ONE inversion"""
    dom = domain(log_n)
    n, p = len(dom), len(points)
    ks = [None] * p
    d = [[(dom[x] - t) % R for t in points] for x in range(n)]
    for x in range(n):
        for j in range(p):
            if d[x][j] == 0:
                ks[j] = x
                if wrong != "vanishing_factor_zero":
                    d[x][j] = 1
    assert [k is not None for k in ks] == [on_domain(t, log_n) for t in points]      # the host's verdict and the lanes' report agree
    P = []
    for x in range(n):
        v = 1
        for j in range(p):
            v = v * d[x][j] % R
        P.append(v)
    A, B = [1] * n, [1] * n                                          # exclusive prefix and suffix products
    for x in range(1, n):
        A[x] = A[x - 1] * P[x - 1] % R
    for x in range(n - 2, -1, -1):
        B[x] = B[x + 1] * P[x + 1] % R
    total_inv = inv(A[n - 1] * P[n - 1] % R)
    out = []
    for x in range(n):
        ip = A[x] * B[x] % R * total_inv % R
        row = []
        for j in range(p):
            co = 1
            for l in range(p):
                if l != j:
                    co = co * d[x][l] % R
            row.append(ip * co % R)
        out.append(row)
    return out, ks


# ---------------------------------------------------------------------------------------------- step 2
def sums(vals, log_n, points, masks, iv, ks):
    """S[i][j] = sum_{x != k_j} f_i[x] omega^x / d_xj for bit j of masks[i], 0 elsewhere"""
    dom = domain(log_n)
    out = []
    for f, m in zip(vals, masks):
        row = [0] * len(points)
        for j in km.members(m, len(points)):
            row[j] = sum(f[x] * dom[x] % R * iv[x][j] for x in range(len(dom)) if x != ks[j]) % R
        out.append(row)
    return out


def evaluations(vals, log_n, points, masks, S, ks):
    return [[0 if not (m >> j) & 1 else f[ks[j]] if ks[j] is not None else S[i][j] * eval_scale(points[j], log_n) % R
             for j in range(len(points))] for i, (f, m) in enumerate(zip(vals, masks))]


# ---------------------------------------------------------------------------------------------- step 3
def at_domain_point(t, ms, g, log_n):
    return (-(ms - g * rest_sum(log_n)) * inv(t)) % R


def quotient_values(vals, log_n, points, coef, g=None, wrong=None):
    """the N values of sum_j D_{t_j}[sum_i coef[i][j] f_i]; g: the values G_j(t_j), found here when None"""
    n, p = 1 << log_n, len(points)
    iv, ks = inverses(log_n, points, wrong)
    masks = [sum(1 << j for j in range(p) if row[j]) for row in coef]
    S = sums(vals, log_n, points, masks, iv, ks)
    if g is None:
        y = evaluations(vals, log_n, points, masks, S, ks)
        g = [sum(coef[i][j] * y[i][j] for i in range(len(vals))) % R for j in range(p)]
    out = []
    for x in range(n):
        acc = 0
        for j in range(p):
            G = sum(coef[i][j] * vals[i][x] for i in range(len(vals)) if coef[i][j]) % R
            if x == ks[j] and wrong != "ordinary_at_k":
                acc += at_domain_point(points[j], sum(coef[i][j] * S[i][j] for i in range(len(vals))) % R, g[j], log_n)
            else:
                acc += (G - g[j]) * iv[x][j]
        out.append(acc % R)
    return out


def opening(vals, log_n, points, sets, gamma, u, wrong=None):
    """what plk_kzg_open_multi_values_dev computes: evaluations, the values of h and of the second quotient"""
    p = len(points)
    iv, ks = inverses(log_n, points, wrong)
    S = sums(vals, log_n, points, sets, iv, ks)
    y = evaluations(vals, log_n, points, sets, S, ks)
    mat = km.matrix(points, sets, gamma)
    if wrong == "g_without_weights":
        g = [sum(pow(gamma, i, R) * y[i][j] for i in range(len(vals)) if (sets[i] >> j) & 1) % R for j in range(p)]
    else:
        g = [sum(mat[i][j] * y[i][j] for i in range(len(vals))) % R for j in range(p)]
    h = quotient_values(vals, log_n, points, mat, g, wrong)
    c, z_t = km.c_values(points, sets, gamma, u)
    v = 0 if wrong == "value_at_u_zero" else sum(ci * km.r_at(points, m, row, u) for ci, m, row in zip(c, sets, y)) % R
    q2 = quotient_values(list(vals) + [h], log_n, [u], [[x] for x in c] + [[(-z_t) % R]], [v], wrong)
    return {"evals": y, "h": h, "q2": q2, "g": g, "v": v, "ks": ks, "S": S}


# ---------------------------------------------------------------------------------------------- the case tables
def directed_points(log_n):
    """point lists that put points on the domain: alone, two of them, mixed with points off it, all of them"""
    w = km.omega(log_n)
    n = 1 << log_n
    on = [pow(w, k, R) for k in sorted({0, 1 % n, n // 2, n - 1})]
    return [[on[0]], [on[-1], km.TAU], [0, on[len(on) // 2], 5], on[:8], (on + [0, km.TAU, 7, 9])[:8]]


MODEL_LOG_SIZES = (1, 3, 5)
