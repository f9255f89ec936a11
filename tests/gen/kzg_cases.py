"""Python-integer model of the KZG opening helpers (plonkit_amd/csrc/kzg.hip) and the case tables of their tests.

Everything here is plain modular arithmetic on canonical residues: interpolation (a recursive radix-2 transform), synthetic division by
(x - z), the barycentric evaluation from values, the quotient (f - y) / (x - z) in values with its in-domain position, and deliberately
wrong variants of the latter that tests/test_kzg_cases_host.py uses to show that the cases discriminate.  No numpy, no oracle: the host
test holds this model against the oracle, the GPU test holds the device against both."""
import random

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
ROOT28 = pow(7, (R - 1) >> 28, R)                                # omega_{2^28}, the library's convention


def omega(log_n):
    return pow(ROOT28, 1 << (28 - log_n), R)


def domain(log_n):
    w, out, x = omega(log_n), [], 1
    for _ in range(1 << log_n):
        out.append(x)
        x = x * w % R
    return out


def _fft(a, w):
    n = len(a)
    if n == 1:
        return a[:]
    ev, od = _fft(a[0::2], w * w % R), _fft(a[1::2], w * w % R)
    out, x = [0] * n, 1
    for i in range(n // 2):
        t = x * od[i] % R
        out[i] = (ev[i] + t) % R
        out[i + n // 2] = (ev[i] - t) % R
        x = x * w % R
    return out


def evaluate_on_domain(coeffs, log_n):
    c = list(coeffs) + [0] * ((1 << log_n) - len(coeffs))
    return _fft(c, omega(log_n))


def interpolate(values, log_n):
    """the coefficients of the polynomial of degree < N with these values on the domain"""
    n_inv = pow(1 << log_n, -1, R)
    return [v * n_inv % R for v in _fft(list(values), pow(omega(log_n), -1, R))]


def horner(coeffs, z):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % R
    return acc


def divide_by_linear(coeffs, z):
    """(p(x) - p(z)) / (x - z): len(coeffs) coefficients, the top one zero (the library's and the oracle's convention)"""
    n, q, acc = len(coeffs), [0] * len(coeffs), 0
    for k in range(n - 1, 0, -1):
        acc = (acc * z + coeffs[k]) % R
        q[k - 1] = acc
    return q


def domain_index(log_n, z):
    """k with z = omega^k, or None"""
    if pow(z, 1 << log_n, R) != 1:
        return None
    return domain(log_n).index(z)


def evaluate_values(values, log_n, z):
    """f(z) from the values: f_k inside the domain, the barycentric formula outside"""
    k = domain_index(log_n, z)
    if k is not None:
        return values[k]
    n = 1 << log_n
    s = sum(f * w % R * pow(z - w, -1, R) for f, w in zip(values, domain(log_n))) % R
    return (pow(z, n, R) - 1) * pow(n, -1, R) % R * s % R


def in_domain_position(values, log_n, k, y):
    """q(omega^k) = sum_{i != k} (f_i - y) omega^i / (z (z - omega^i)), z = omega^k"""
    dom = domain(log_n)
    z = dom[k]
    return sum((f - y) * w % R * pow(z * (z - w) % R, -1, R) for i, (f, w) in enumerate(zip(values, dom)) if i != k) % R


WRONG_VARIANTS = ("no_substitution", "fk_from_formula", "no_omega_factor", "k_off_by_one")


def quotient_values(values, log_n, z, y=None, wrong=None):
    """the N values of (f - y) / (x - z); y = None: f(z).  wrong: one of WRONG_VARIANTS, what a broken kernel would compute."""
    dom, n = domain(log_n), 1 << log_n
    k = domain_index(log_n, z)
    if wrong == "fk_from_formula" and k is not None and y is None:
        # the barycentric formula evaluated blindly at a domain point: (z^N - 1) = 0 kills it
        y = 0
    if y is None:
        y = evaluate_values(values, log_n, z)
    if k is None:
        return [(f - y) * pow(w - z, -1, R) % R for f, w in zip(values, dom)]
    if wrong == "no_substitution":
        return [0] * n                                           # one zero denominator: every prefix x suffix product vanishes
    kk = (k + 1) % n if wrong == "k_off_by_one" else k
    out = [0] * n
    for i in range(n):
        if i != kk:
            d = (dom[i] - z) % R
            out[i] = (values[i] - y) * pow(d, -1, R) % R if d else 0
    if wrong == "no_omega_factor":
        out[kk] = sum((f - y) * pow(z * (z - w) % R, -1, R) for i, (f, w) in enumerate(zip(values, dom)) if i != kk) % R
    elif wrong == "k_off_by_one":
        out[kk] = sum((f - y) * w % R * pow(dom[kk] * (dom[kk] - w) % R, -1, R) for i, (f, w) in enumerate(zip(values, dom)) if i != kk) % R
    else:
        out[kk] = in_domain_position(values, log_n, k, y)
    return out


# ---------------------------------------------------------------------------------------------- the case tables
HELPER_LOG_NS = (1, 2, 3, 8, 11, 12, 16)                         # 2^11 = one scan block, 2^12 = two
LARGE_LOG_N = 22                                                 # past the 1024 block totals of one launch of the totals scan
DOMAIN_KS = (0, 1, 2047, 2048, "N-1")
POLY_KINDS = ("zero", "constant", "all_r_minus_1", "x_minus_z", "random")
MODEL_LOG_NS = (1, 2, 3, 4)                                      # where the quadratic model above is affordable


def z_cases(log_n, seed=1):
    """name -> z: random, 0, 1, r - 1, omega^k where it exists, a primitive 2N-th root (off the domain by the narrowest margin), 42"""
    n = 1 << log_n
    rng = random.Random(1000 * log_n + seed)
    out = {"random": rng.randrange(2, R), "0": 0, "1": 1, "r-1": R - 1, "42": 42}
    for k in DOMAIN_KS:
        kk = n - 1 if k == "N-1" else k
        if kk < n:
            out["omega^%s" % k] = pow(omega(log_n), kk, R)
    if log_n < 28:
        out["2N-th root"] = omega(log_n + 1)
    return out


def poly_values(kind, log_n, z, seed=2):
    """the N values of the case polynomial"""
    n = 1 << log_n
    if kind == "zero":
        return [0] * n
    if kind == "constant":
        return [7] * n
    if kind == "all_r_minus_1":
        return [R - 1] * n
    if kind == "x_minus_z":
        return [(w - z) % R for w in domain(log_n)]
    rng = random.Random(77 * log_n + seed)
    return [rng.randrange(R) for _ in range(n)]
