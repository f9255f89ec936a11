"""Python-integer model of the multi-point openings (plonkit_amd/csrc/kzg_multi.hip, kzg_multi_plan.h; Boneh-Drake-Fisch-Gabizon 2020)
and the case tables of their tests.

Plain modular arithmetic on canonical residues, lists of coefficients, no numpy, no oracle.  The first quotient h is computed BY THE
DEFINITION — interpolate r_i, subtract, long-divide by Z_{S_i} — and, separately, by the grouped formula the kernel implements; the host
test holds the two against each other, the verifier's equation in the exponent (tau known), and shows that three plausible wrong
arrangements fail it."""
import random

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
ROOT28 = pow(7, (R - 1) >> 28, R)
TAU = 42


def omega(log_n):
    return pow(ROOT28, 1 << (28 - log_n), R)


# ---------------------------------------------------------------------------------------------- polynomials as lists, lowest first
def horner(c, z):
    acc = 0
    for a in reversed(c):
        acc = (acc * z + a) % R
    return acc


def padd(a, b):
    n = max(len(a), len(b))
    return [((a[k] if k < len(a) else 0) + (b[k] if k < len(b) else 0)) % R for k in range(n)]


def pscale(a, s):
    return [x * s % R for x in a]


def pmul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R
    return out


def pdivmod(a, d):
    """long division by a monic d: (quotient, remainder)"""
    assert d[-1] == 1
    a, q = list(a), [0] * max(len(a) - len(d) + 1, 1)
    for k in range(len(a) - len(d), -1, -1):
        c = a[k + len(d) - 1]
        q[k] = c
        if c:
            for j, y in enumerate(d):
                a[k + j] = (a[k + j] - c * y) % R
    return q, a[:len(d) - 1]


def z_poly(points):
    out = [1]
    for t in points:
        out = pmul(out, [(-t) % R, 1])
    return out


def members(mask, npoints):
    return [j for j in range(npoints) if (mask >> j) & 1]


def interpolate(points, values):
    """the polynomial of degree < len(points) through (points[k], values[k])"""
    out = [0] * len(points)
    for k, (t, y) in enumerate(zip(points, values)):
        others = [s for l, s in enumerate(points) if l != k]
        den = 1
        for s in others:
            den = den * (t - s) % R
        out = padd(out, pscale(z_poly(others), y * pow(den, -1, R) % R))
    return out


def divide_by_linear(c, z):
    """D_z[c] = (c - c(z)) / (x - z): len(c) coefficients, the top one zero"""
    n, q, acc = len(c), [0] * len(c), 0
    for k in range(n - 1, 0, -1):
        acc = (acc * z + c[k]) % R
        q[k - 1] = acc
    return q


# ---------------------------------------------------------------------------------------------- the scheme
WRONG = ("gamma_by_point", "no_weights", "z_of_the_set")


def weights(points, sets):
    """w[i][j] = 1 / prod_{l in S_i, l != j} (t_j - t_l) for j in S_i, 0 elsewhere"""
    p = len(points)
    out = []
    for mask in sets:
        row = [0] * p
        for j in members(mask, p):
            den = 1
            for l in members(mask, p):
                if l != j:
                    den = den * (points[j] - points[l]) % R
            row[j] = pow(den, -1, R)
        out.append(row)
    return out


def matrix(points, sets, gamma, wrong=None):
    """gamma^i w_ij: the matrix of the first quotient"""
    w = weights(points, sets)
    out = []
    for i, mask in enumerate(sets):
        row = [0] * len(points)
        for j in members(mask, len(points)):
            g = pow(gamma, j if wrong == "gamma_by_point" else i, R)
            row[j] = g * (1 if wrong == "no_weights" else w[i][j]) % R
        out.append(row)
    return out


def quotient_multi(polys, points, coef):
    """out[k] = sum_j sum_{l > k} G_j[l] t_j^(l-k-1), G_j = sum_i coef[i][j] f_i: what plk_poly_quotient_multi_dev computes"""
    n = len(polys[0])
    out = [0] * n
    for j, t in enumerate(points):
        g = [0] * n
        for i, f in enumerate(polys):
            if coef[i][j]:
                g = padd(g, pscale(f, coef[i][j]))
        out = padd(out, divide_by_linear(g, t))
    return out


def h_by_definition(polys, points, sets, gamma):
    """sum_i gamma^i (f_i - r_i) / Z_{S_i}: interpolation and long division; every remainder must vanish"""
    n = len(polys[0])
    out = [0] * n
    for i, (f, mask) in enumerate(zip(polys, sets)):
        s = [points[j] for j in members(mask, len(points))]
        r = interpolate(s, [horner(f, t) for t in s])
        num = padd(f, pscale(r, R - 1))
        q, rem = pdivmod(num, z_poly(s)) if len(num) > len(s) else ([0], num)
        assert not any(rem), "f_i - r_i is divisible by Z_{S_i}"
        out = padd(out, pscale(q, pow(gamma, i, R)))
    return (out + [0] * n)[:n]


def h_grouped(polys, points, sets, gamma, wrong=None):
    return quotient_multi(polys, points, matrix(points, sets, gamma, wrong))


def z_at(points, idx, u):
    out = 1
    for j in idx:
        out = out * (u - points[j]) % R
    return out


def c_values(points, sets, gamma, u, wrong=None):
    """c_i = gamma^i Z_{T \\ S_i}(u), and Z_T(u)"""
    p = len(points)
    out = []
    for i, mask in enumerate(sets):
        idx = members(mask, p) if wrong == "z_of_the_set" else [j for j in range(p) if not (mask >> j) & 1]
        out.append(pow(gamma, i, R) * z_at(points, idx, u) % R)
    return out, z_at(points, range(p), u)


def r_at(points, mask, evals_row, u):
    """r_i(u) from the evaluations on S_i (Lagrange)"""
    idx = members(mask, len(points))
    out = 0
    for j in idx:
        num, den = 1, 1
        for l in idx:
            if l != j:
                num, den = num * (u - points[l]) % R, den * (points[j] - points[l]) % R
        out = (out + evals_row[j] * num % R * pow(den, -1, R)) % R
    return out


def evaluations(polys, points, sets):
    """[count][npoints], zero outside the sets"""
    return [[horner(f, t) if (mask >> j) & 1 else 0 for j, t in enumerate(points)] for f, mask in zip(polys, sets)]


def second_quotient(polys, h, points, sets, gamma, u, wrong=None):
    """L / (x - u) = D_u[sum_i c_i f_i - Z_T(u) h]"""
    c, z_t = c_values(points, sets, gamma, u, wrong)
    return quotient_multi(list(polys) + [h], [u], [[x] for x in c] + [[(-z_t) % R]])


def second_quotient_by_definition(polys, h, points, sets, gamma, u):
    """L = sum_i c_i (f_i - r_i(u)) - Z_T(u) h with L(u) = 0, long-divided by (x - u)"""
    c, z_t = c_values(points, sets, gamma, u)
    ev = evaluations(polys, points, sets)
    n = len(polys[0])
    L = pscale(h, (-z_t) % R)
    for i, f in enumerate(polys):
        g = list(f)
        g[0] = (g[0] - r_at(points, sets[i], ev[i], u)) % R
        L = padd(L, pscale(g, c[i]))
    assert horner(L, u) == 0
    q, rem = pdivmod(L, [(-u) % R, 1]) if n > 1 else ([0], L)
    assert not any(rem)
    return (q + [0] * n)[:n]


def opening(polys, points, sets, gamma, u, wrong=None):
    """what the prover outputs and what the verifier derives, as integers; w and w2 are the exponents of W and W' under tau"""
    h = h_grouped(polys, points, sets, gamma, wrong)
    q2 = second_quotient(polys, h, points, sets, gamma, u, wrong)
    c, z_t = c_values(points, sets, gamma, u, wrong)
    ev = evaluations(polys, points, sets)
    return {"evals": ev, "h": h, "q2": q2, "c": c, "z_t": z_t, "r_u": [r_at(points, m, row, u) for m, row in zip(sets, ev)],
            "w": horner(h, TAU), "w2": horner(q2, TAU)}


def verifier_exponent(commitments, points, sets, evals, gamma, u, w, w2, tau=TAU):
    """log_G of F + u W' - tau W' with every group element given by its exponent: zero exactly when the pairing product is one"""
    c, z_t = c_values(points, sets, gamma, u)
    F = (-z_t * w) % R
    for i, cm in enumerate(commitments):
        F = (F + c[i] * (cm - r_at(points, sets[i], evals[i], u))) % R
    return (F + (u - tau) * w2) % R


# ---------------------------------------------------------------------------------------------- the case tables
def check_sets(points, sets):
    """None, or why the library refuses these sets"""
    if len(set(points)) != len(points):
        return "duplicate point"
    used = 0
    for m in sets:
        if m == 0:
            return "empty set"
        if m >> len(points):
            return "bit above"
        used |= m
    return None if used == (1 << len(points)) - 1 else "unused point"


def singleton_masks(m, p):
    """polynomial i at point i mod p alone (m >= p, so that every point is used)"""
    assert m >= p
    return [1 << (i % p) for i in range(m)]


def all_masks(m, p):
    return [(1 << p) - 1] * m


def plonk_like_masks(m):
    """all at t_0, two also at t_1, one also at t_2 (m >= 3)"""
    out = [1] * m
    out[m - 1] |= 2
    out[m - 2] |= 2
    out[0] |= 4
    return out


def random_masks(m, p, seed):
    rng = random.Random(seed)
    out = [rng.randrange(1, 1 << p) for _ in range(m)]
    for j in range(p):                                              # every point is used
        out[j % m] |= 1 << j
    return out


def point_cases(log_n, p, seed=3):
    """p distinct points drawn from: 0, 1, r - 1, 42, omega^k of the size, random"""
    rng = random.Random(1000 * log_n + 10 * p + seed)
    w = omega(log_n) if log_n else 1
    pool = [0, 1, R - 1, TAU, pow(w, 3, R), pow(w, (1 << log_n) - 1, R)]
    out = []
    for t in pool:
        if t not in out:
            out.append(t)
    while len(out) < 8:
        t = rng.randrange(2, R)
        if t not in out:
            out.append(t)
    rng.shuffle(out)
    return out[:p]


POLY_KINDS = ("zero", "constant", "all_r_minus_1", "random")


def poly(kind, n, seed):
    if kind == "zero":
        return [0] * n
    if kind == "constant":
        return [7] + [0] * (n - 1)
    if kind == "all_r_minus_1":
        return [R - 1] * n
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


MODEL_SIZES = (1, 2, 3, 7, 24, 32)                                 # where the quadratic model is affordable
HOST_SHAPES = ((1, 1), (3, 2), (8, 4), (32, 8))                    # (m, p)


def mask_families(m, p, seed=5):
    """name -> masks for m polynomials and p points (families that do not fit the shape are left out)"""
    out = {"all": all_masks(m, p), "random": random_masks(m, p, seed)}
    if m >= p:
        out["singletons"] = singleton_masks(m, p)
    if m >= 3 and p == 3:
        out["plonk_like"] = plonk_like_masks(m)
    return out
