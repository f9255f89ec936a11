"""Python-integer model of the one-pass openings on the whole domain (plonkit_amd/csrc/kzg_all.hip, kzg_all_plan.h) and its case tables.

Group elements are modelled by their discrete logarithms: the key point s_j = tau^j G is the integer tau^j mod r, a sum of points a sum of
integers, a scalar multiple a product.  With that, everything the device does is plain modular arithmetic:
  h by its definition     h_k = sum_{j=0}^{N-2-k} f_{k+1+j} s_j  (k <= N - 2),  h_{N-1} = 0
  the two arrangements    c_m = f_{m+1} for m <= N - 2;  t_0 = s_0, t_{2N-j} = s_j for 1 <= j <= N - 2;  zero / identity elsewhere
  the 2N correlation      h = the first N entries of iDFT_2N(DFT_2N(c) o DFT_2N(t)), 1 / 2N included
  the openings            pi_i = DFT_N(h)_i, against the definition (f(tau) - f(omega^i)) / (tau - omega^i)
and deliberately wrong variants of the correlation that tests/test_fk20_cases_host.py uses to show that the cases discriminate.
No numpy, no oracle."""
import random

from tests.gen.kzg_cases import R, horner, omega

NONE = None                                                      # "zero" in c, "the identity" in t


def dft(v, w):
    """out[i] = sum_j v[j] w^(i j): the definition, quadratic (the model runs up to 64 points)"""
    n = len(v)
    pw = [pow(w, e, R) for e in range(n)]
    return [sum(v[j] * pw[i * j % n] for j in range(n)) % R for i in range(n)]


def idft(v, w):
    n_inv = pow(len(v), -1, R)
    return [x * n_inv % R for x in dft(v, pow(w, -1, R))]


def key(tau, count):
    return [pow(tau, j, R) for j in range(count)]


def quotient_commitments(f, tau):
    """h_0 .. h_{N-1} by their definition"""
    n = len(f)
    s = key(tau, n)
    return [sum(f[k + 1 + j] * s[j] for j in range(n - 1 - k)) % R for k in range(n - 1)] + [0]


def c_sources(log_n):
    """src[m] = the index of the coefficient at c[m], or NONE; length 2N"""
    n = 1 << log_n
    src = [NONE] * (2 * n)
    for i in range(1, n):
        src[i - 1] = i
    return src


def t_sources(log_n, wrong=None):
    """src[m] = the index of the key point at t[m], or NONE; length 2N"""
    n = 1 << log_n
    src = [NONE] * (2 * n)
    if n >= 2:
        src[0] = 0
    for j in range(1, n - 1):
        src[j if wrong == "t_swapped" else 2 * n - j] = j
    return src


def arrange(src, values):
    return [0 if s is NONE else values[s] for s in src]


WRONG_VARIANTS = ("t_swapped", "no_scale", "upper_half")


def correlation_h(f, tau, log_n, wrong=None):
    """h through the 2N correlation; wrong: what a broken arrangement would compute"""
    n = 1 << log_n
    w2 = omega(log_n + 1)
    c = arrange(c_sources(log_n), f)
    t = arrange(t_sources(log_n, wrong), key(tau, n))
    prod = [a * b % R for a, b in zip(dft(c, w2), dft(t, w2))]
    full = dft(prod, pow(w2, -1, R)) if wrong == "no_scale" else idft(prod, w2)
    return full[n:] if wrong == "upper_half" else full[:n]


def openings(f, tau, log_n, wrong=None):
    """pi_i as discrete logarithms, through the correlation and the forward transform at N"""
    return dft(correlation_h(f, tau, log_n, wrong), omega(log_n))


def openings_by_definition(f, tau, log_n):
    """(f(tau) - f(omega^i)) / (tau - omega^i); tau must not lie on the domain"""
    w, ft = omega(log_n), horner(f, tau)
    out = []
    for i in range(1 << log_n):
        z = pow(w, i, R)
        out.append((ft - horner(f, z)) * pow(tau - z, -1, R) % R)
    return out


# ---------------------------------------------------------------------------------------------- the case tables
MODEL_LOG_NS = (0, 1, 2, 3, 4, 5)                                # N = 1 .. 32
POLY_KINDS = ("zero", "constant", "top_only", "f1_only", "random")
TAUS = (42, 0x1f2e3d4c5b6a79880112233445566778899aabbccddeeff0011223344556677 % R)


def poly(kind, log_n, seed=3):
    """the N coefficients of the case polynomial"""
    n = 1 << log_n
    rng = random.Random(101 * log_n + seed)
    f = [0] * n
    if kind == "constant":
        f[0] = 7
    elif kind == "top_only":
        f[n - 1] = rng.randrange(1, R)
    elif kind == "f1_only":
        if n > 1:
            f[1] = rng.randrange(1, R)
    elif kind == "random":
        f = [rng.randrange(R) for _ in range(n)]
    return f
