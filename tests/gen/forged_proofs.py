"""Forged proofs for the verifier's edges (pure Python on the oracle).

Every key of this project has a known trapdoor tau, and a test may choose its own.  With tau known, a "proof" that VERIFIES can be built
forward through the transcript from data chosen at will, with every commitment given as its discrete logarithm to the generator G
(0 = the point at infinity):

  1. everything up to the challenge v is free: the key's 11 commitments, the wires, Z, the quotient parts, every evaluation but t(z);
  2. t(z) is solved from the equation at z;
  3. the aggregate of verify_commitments (`agg` plus the generator term, in verify.cpp's names) is A0 + u A1, and both parts are fixed
     before u is drawn;
  4. W_z = -A0 / (z - tau) and W_zw = -A1 / (z omega - tau).  Neither depends on u, and then pg + tau px = O.

This reaches what the prover never produces: points at infinity, zero scalars, equal and opposite consecutive terms, domain sizes 2 and 2^28,
trapdoors other than 42.  The broken variants keep the equation at z true, so they too reach the group arithmetic and the pairing:

  "plus_g"   W_z + G                                  invalid
  "px_inf"   W_z = W_zw = O          px = O           invalid unless pg = O too
  "pg_inf"   W_z = -A0 / z, A1 = 0   pg = O           invalid unless px = O too   (needs Z = w_3 = O and z(z omega) = d(z omega) = 0)

forge() checks every result against oracle.plonk_oracle.verify before it returns: a case that does not forge is an error.
"""
import os
import random
from collections import namedtuple

import numpy as np

from oracle import oracle_lib as ol
from oracle import plonk_oracle as po
from oracle.oracle_lib import R_MOD, Q_MOD

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
G2_INF = b"\x40" + b"\x00" * 127
VARIANTS = (None, "plus_g", "px_inf", "pg_inf")

Forged = namedtuple("Forged", "vk proof pg px valid")        # pg, px: discrete logarithms of the verifier's two pairing arguments


# ------------------------------------------------------------------------------------------------ G1 from logarithms
_G1_CACHE = {}


def g1_of(c):
    """c G as Montgomery affine limbs; 0 = the point at infinity"""
    c %= R_MOD
    if c not in _G1_CACHE:
        _G1_CACHE[c] = np.zeros(8, dtype=np.uint64) if c == 0 else ol.g1_mul(ol.g1_generator(), c)
    return _G1_CACHE[c]


# ------------------------------------------------------------------------------------------------ G2: bytes and the twist
def golden_g2():
    """(G2, 42 G2) as their 128 file bytes each, from the golden verification key"""
    raw = open(os.path.join(GOLDEN, "vk.bin"), "rb").read()[-256:]
    return raw[:128], raw[128:]


def g2_neg_bytes(b):
    """-Q: both halves of y replaced by q - y"""
    if b == G2_INF:
        return b
    y1, y0 = int.from_bytes(b[64:96], "big"), int.from_bytes(b[96:128], "big")
    return b[:64] + ((Q_MOD - y1) % Q_MOD).to_bytes(32, "big") + ((Q_MOD - y0) % Q_MOD).to_bytes(32, "big")


# Fq2 = Fq[i] / (i^2 + 1) as (c0, c1); the file order of a coordinate is c1 then c0
def _f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q_MOD, (a[0] * b[1] + a[1] * b[0]) % Q_MOD)


def _f2_sub(a, b):
    return ((a[0] - b[0]) % Q_MOD, (a[1] - b[1]) % Q_MOD)


def _f2_inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % Q_MOD, -1, Q_MOD)
    return (a[0] * n % Q_MOD, (Q_MOD - a[1]) * n % Q_MOD)


def _g2_decode(b):
    c = [int.from_bytes(b[32 * k:32 * k + 32], "big") for k in range(4)]
    return (c[1], c[0]), (c[3], c[2])


def _g2_encode(p):
    if p is None:
        return G2_INF
    (x0, x1), (y0, y1) = p
    return b"".join(v.to_bytes(32, "big") for v in (x1, x0, y1, y0))


def _g2_add(p, q):
    """affine addition on the twist y^2 = x^3 + 3 / (9 + i); None = infinity"""
    if p is None:
        return q
    if q is None:
        return p
    (px, py), (qx, qy) = p, q
    if px == qx:
        if py != qy or py == (0, 0):
            return None
        x2 = _f2_mul(px, px)
        m = _f2_mul(((3 * x2[0]) % Q_MOD, (3 * x2[1]) % Q_MOD), _f2_inv(((2 * py[0]) % Q_MOD, (2 * py[1]) % Q_MOD)))
    else:
        m = _f2_mul(_f2_sub(qy, py), _f2_inv(_f2_sub(qx, px)))
    x3 = _f2_sub(_f2_sub(_f2_mul(m, m), px), qx)
    return x3, _f2_sub(_f2_mul(m, _f2_sub(px, x3)), py)


def g2_mul_bytes(b, k):
    """k Q by double-and-add over plain integers, on the 128 file bytes"""
    p, acc = _g2_decode(b), None
    for bit in bin(k % R_MOD)[2:]:
        acc = _g2_add(acc, acc)
        if bit == "1":
            acc = _g2_add(acc, p)
    return _g2_encode(acc)


_TWIST_CHECKED = []


def g2_pair(tau):
    """G2 || tau G2.  tau = 1 and tau = r - 1 need no G2 arithmetic; any other goes through the twist code, which must first
    reproduce the golden key's second point from 42 and the negation from r - 1"""
    g, g42 = golden_g2()
    tau %= R_MOD
    if tau == 1:
        return g + g
    if tau == R_MOD - 1:
        return g + g2_neg_bytes(g)
    if tau == 42:
        return g + g42
    if not _TWIST_CHECKED:
        assert g2_mul_bytes(g, 42) == g42, "the twist arithmetic does not reproduce 42 G2 of the golden key"
        assert g2_mul_bytes(g, R_MOD - 1) == g2_neg_bytes(g) and g2_mul_bytes(g, R_MOD) == G2_INF
        _TWIST_CHECKED.append(True)
    return g + g2_mul_bytes(g, tau)


# ------------------------------------------------------------------------------------------------ the forger
def forge_record(key_dlogs, n, inputs, wires, Z, t, wz, wzw, z_zw, sz, r_z=None, tau=42, variant=None, g2=None):
    """-> Forged(vk bytes, proof bytes, log pg, log px, valid).

    key_dlogs  11 logarithms: selectors q_a q_b q_c q_d q_m q_const, q_d_next, sigma_0..3
    n          the key's n (domain size N = n + 1, a power of two)
    inputs     public inputs (their count is the key's num_inputs)
    wires, Z, t  logarithms of the 4 wire commitments, the grand product, the 4 quotient parts
    wz, wzw, z_zw, sz, r_z  the evaluations a(z)..d(z), d(z omega), z(z omega), sigma_0..2(z), r(z) (None = 0); t(z) is solved
    variant    None or one of the broken variants of the module's docstring
    g2         256 bytes that replace G2 || tau G2 in the key (a point at infinity, which the oracle has no model of):
               `valid` is then left None, and the caller decides from pg and px
    """
    assert len(key_dlogs) == 11 and len(wires) == 4 and len(t) == 4 and len(wz) == 4 and len(sz) == 3 and variant in VARIANTS
    N = n + 1
    log_n = N.bit_length() - 1
    assert N == 1 << log_n and 1 <= log_n <= 28
    key = [c % R_MOD for c in key_dlogs]
    r_z = 0 if r_z is None else r_z % R_MOD
    om = ol.omega(log_n)

    vk = po.VerificationKey()
    vk.n, vk.num_inputs = n, len(inputs)
    vk.selector_commitments = [g1_of(c) for c in key[:6]]
    vk.next_step_selector_commitments = [g1_of(key[6])]
    vk.permutation_commitments = [g1_of(c) for c in key[7:]]
    vk.non_residues = list(po.NON_RESIDUES[1:])
    vk.g2_raw = g2 if g2 is not None else g2_pair(tau)
    assert len(vk.g2_raw) == 256

    P = po.Proof()
    P.n, P.inputs = n, [x % R_MOD for x in inputs]
    P.wire_commitments = [g1_of(c) for c in wires]
    P.grand_product_commitment = g1_of(Z)
    P.quotient_poly_commitments = [g1_of(c) for c in t]
    P.wire_values_at_z = [x % R_MOD for x in wz]
    P.wire_values_at_z_omega = [wzw % R_MOD]
    P.permutation_polynomials_at_z = [x % R_MOD for x in sz]
    P.grand_product_at_z_omega = z_zw % R_MOD
    P.linearization_polynomial_at_z = r_z
    wz, sz, wzw, z_zw = P.wire_values_at_z, P.permutation_polynomials_at_z, P.wire_values_at_z_omega[0], P.grand_product_at_z_omega

    # the transcript, step for step as po.verify walks it
    tr = po.Transcript()
    for x in P.inputs:
        tr.absorb_fr(x)
    for c in P.wire_commitments:
        tr.absorb_g1(c)
    beta, gamma = tr.challenge(), tr.challenge()
    tr.absorb_g1(P.grand_product_commitment)
    alpha = tr.challenge()
    for c in P.quotient_poly_commitments:
        tr.absorb_g1(c)
    z = tr.challenge()
    zN = pow(z, N, R_MOD)
    assert zN != 1
    lag = [pow(om, i, R_MOD) * (zN - 1) % R_MOD * pow(N * (z - pow(om, i, R_MOD)) % R_MOD, -1, R_MOD) % R_MOD
           for i in range(max(len(P.inputs), 1))]
    # t(z) (z^N - 1) = r(z) + PI(z) - alpha z(z omega) prod_j (..) (gamma + d) - alpha^2 L_0(z)
    rhs = r_z
    for i, x in enumerate(P.inputs):
        rhs = (rhs + lag[i] * x) % R_MOD
    zpart = z_zw
    for j in range(3):
        zpart = zpart * ((sz[j] * beta + gamma + wz[j]) % R_MOD) % R_MOD
    zpart = zpart * ((gamma + wz[3]) % R_MOD) % R_MOD * alpha % R_MOD
    rhs = (rhs - zpart - lag[0] * alpha * alpha) % R_MOD
    t_z = rhs * pow(zN - 1, -1, R_MOD) % R_MOD
    P.quotient_polynomial_at_z = t_z
    for x in wz + [wzw] + sz:
        tr.absorb_fr(x)
    tr.absorb_fr(t_z)
    tr.absorb_fr(r_z)
    tr.absorb_fr(z_zw)
    v = tr.challenge()

    def agg(u):
        """the logarithm of verify_commitments' aggregate with the generator term, for a given u: linear in u"""
        d = (key[5] + sum(key[j] * wz[j] for j in range(4)) + key[4] * wz[0] * wz[1] + key[6] * wzw) % R_MOD
        gz = (z * beta + wz[0] + gamma) % R_MOD
        for j in range(3):
            gz = gz * ((z * vk.non_residues[j] * beta + gamma + wz[j + 1]) % R_MOD) % R_MOD
        gz = (gz * alpha + lag[0] * alpha * alpha) % R_MOD
        gzw = pow(v, 9, R_MOD) * u % R_MOD
        last = 1
        for j in range(3):
            last = last * ((beta * sz[j] + gamma + wz[j]) % R_MOD) % R_MOD
        last = last * beta % R_MOD * z_zw % R_MOD * alpha % R_MOD
        d = ((d + Z * gz - key[10] * last) * v + Z * gzw) % R_MOD
        a = (sum(t[k] * pow(zN, k, R_MOD) for k in range(4)) + d) % R_MOD
        ch = v
        for c in list(wires) + key[7:10]:
            ch = ch * v % R_MOD
            a = (a + c * ch) % R_MOD
        ch = ch * v % R_MOD * v % R_MOD
        a = (a + wires[3] * ch % R_MOD * u) % R_MOD
        ch = v
        val = (t_z + r_z * ch) % R_MOD
        for x in wz + sz:
            ch = ch * v % R_MOD
            val = (val + x * ch) % R_MOD
        ch = ch * v % R_MOD
        val = (val + z_zw * ch % R_MOD * u) % R_MOD
        ch = ch * v % R_MOD
        val = (val + wzw * ch % R_MOD * u) % R_MOD
        return (a - val) % R_MOD

    A0 = agg(0)
    A1 = (agg(1) - A0) % R_MOD
    assert (agg(12345) - A0 - 12345 * A1) % R_MOD == 0
    zw = z * om % R_MOD
    assert (z - tau) % R_MOD and (zw - tau) % R_MOD and z
    W_z = -A0 * pow(z - tau, -1, R_MOD) % R_MOD
    W_zw = -A1 * pow(zw - tau, -1, R_MOD) % R_MOD
    if variant == "plus_g":
        W_z = (W_z + 1) % R_MOD
    elif variant == "px_inf":
        W_z = W_zw = 0
    elif variant == "pg_inf":
        assert A1 == 0, "pg_inf needs Z = w_3 = O and z(z omega) = d(z omega) = 0"
        W_z, W_zw = -A0 * pow(z, -1, R_MOD) % R_MOD, 0
    P.opening_at_z_proof, P.opening_at_z_omega_proof = g1_of(W_z), g1_of(W_zw)
    tr.absorb_g1(P.opening_at_z_proof)
    tr.absorb_g1(P.opening_at_z_omega_proof)
    u = tr.challenge()
    pg = (A0 + u * A1 + z * W_z + zw * u % R_MOD * W_zw) % R_MOD
    px = -(W_z + u * W_zw) % R_MOD
    vk_bytes, proof_bytes = po.write_vk(vk), po.write_proof(P)
    if g2 is not None:
        return Forged(vk_bytes, proof_bytes, pg, px, None)
    valid = (pg + tau * px) % R_MOD == 0
    assert valid or variant is not None, "the forged proof does not satisfy its own pairing equation"
    assert po.verify(po.read_vk(vk_bytes), po.read_proof(proof_bytes), tau) == valid, "the oracle disagrees with the forger's logarithms"
    return Forged(vk_bytes, proof_bytes, pg, px, valid)


def forge(key_dlogs, n, inputs, wires, Z, t, wz, wzw, z_zw, sz, r_z=None, tau=42, **more):
    """-> (vk bytes, proof bytes); see forge_record"""
    f = forge_record(key_dlogs, n, inputs, wires, Z, t, wz, wzw, z_zw, sz, r_z, tau, **more)
    return f.vk, f.proof


def g2_inf_verdict(f, g2):
    """the closed form where a G2 point is at infinity: e(pg, Q0) e(px, Q1) with e(., O) = 1 and e(O, .) = 1"""
    pg_live = f.pg != 0 and g2[:128] != G2_INF
    px_live = f.px != 0 and g2[128:] != G2_INF
    assert not (pg_live and px_live), "both pairings are live: this is the oracle's case"
    return not pg_live and not px_live


# ------------------------------------------------------------------------------------------------ named cases
def random_args(rng, n=(1 << 10) - 1, num_inputs=2, key=None):
    """full-range data for every argument of forge (a dict); `key` fixes the 11 logarithms of the key"""
    fr = lambda: rng.randrange(R_MOD)
    return dict(key_dlogs=list(key) if key is not None else [fr() for _ in range(11)], n=n, inputs=[fr() for _ in range(num_inputs)],
                wires=[fr() for _ in range(4)], Z=fr(), t=[fr() for _ in range(4)], wz=[fr() for _ in range(4)], wzw=fr(), z_zw=fr(),
                sz=[fr() for _ in range(3)], r_z=fr())


def no_wzw(args):
    """the same data with A1 = 0: Z = w_3 = O and z(z omega) = d(z omega) = 0, so that W_zw = O (and "pg_inf" can be forged)"""
    a = dict(args)
    a["Z"], a["wires"], a["wzw"], a["z_zw"] = 0, list(args["wires"][:3]) + [0], 0, 0
    return a


def edge_cases(seed=20261018):
    """name -> keyword arguments of forge_record: the constructions that no prover output reaches.  Deterministic."""
    rng = random.Random(seed)
    fr = lambda: rng.randrange(R_MOD)
    big = R_MOD - 1
    out = {}
    for k, (log_n, ni) in enumerate(((10, 2), (1, 0), (28, 1), (5, 9), (3, 300))):
        out["random_N2^%d_%d_inputs" % (log_n, ni)] = random_args(rng, (1 << log_n) - 1, ni)
    # only points at infinity, N = 2: every product but the generator's is the identity
    zero = dict(key_dlogs=[0] * 11, n=1, inputs=[], wires=[0] * 4, Z=0, t=[0] * 4, wz=[fr() for _ in range(4)], wzw=fr(), z_zw=fr(),
                sz=[fr() for _ in range(3)], r_z=fr())
    out["all_infinity_N2"] = zero
    out["all_infinity_zero_evaluations_N2"] = dict(zero, wz=[0] * 4, wzw=0, z_zw=0, sz=[0] * 3, r_z=0)
    # all selectors equal: consecutive terms of the 23-term sum coincide or cancel
    c, a = fr(), fr()
    same = random_args(rng, 7, 1, key=[c] * 11)
    out["equal_key_doubling_at_step_1"] = dict(same, wz=[a, a, 0, 0])
    out["equal_key_cancellation_at_step_1"] = dict(same, wz=[a, big + 1 - a, 0, 0])
    out["equal_key_doubling_at_step_5"] = dict(same, wz=[0, 0, 0, 1])
    out["equal_key_cancellation_at_step_5"] = dict(same, wz=[0, 0, 0, big])
    # the same group element in two XYZZ representations: 2c with a/2 next to c with a
    half = a * pow(2, -1, R_MOD) % R_MOD
    out["other_representation_doubling"] = dict(same, key_dlogs=[2 * c % R_MOD] + [c] * 10, wz=[half, a, 0, 0])
    out["other_representation_cancellation"] = dict(same, key_dlogs=[2 * c % R_MOD] + [c] * 10, wz=[half, big + 1 - a, 0, 0])
    # the key, the proof and term 22 all on the generator
    out["all_generator"] = dict(random_args(rng, 3, 1, key=[1] * 11), wires=[1] * 4, Z=1, t=[1] * 4)
    out["all_generator_unit_evaluations"] = dict(out["all_generator"], wz=[1] * 4, wzw=1, z_zw=1, sz=[1] * 3, r_z=1, inputs=[1])
    # every evaluation r - 1 on the largest domain
    out["evaluations_r_minus_1_N2^28"] = dict(random_args(rng, (1 << 28) - 1, 1), wz=[big] * 4, wzw=big, z_zw=big, sz=[big] * 3, r_z=big,
                                               inputs=[big])
    # W_zw = O
    out["no_opening_at_z_omega"] = no_wzw(random_args(rng, 15, 1))
    for tau in (1, big, 5):
        out["tau_%s" % ("r_minus_1" if tau == big else tau)] = dict(random_args(rng, 15, 1), tau=tau)
    return out


def broken_cases(seed=20261019):
    """name -> keyword arguments of forge_record whose verdict is invalid although the equation at z holds"""
    rng = random.Random(seed)
    out = {}
    for log_n, ni in ((10, 2), (1, 0), (28, 9)):
        base = random_args(rng, (1 << log_n) - 1, ni)
        out["plus_g_N2^%d" % log_n] = dict(base, variant="plus_g")
        out["px_inf_N2^%d" % log_n] = dict(base, variant="px_inf")
        out["pg_inf_N2^%d" % log_n] = dict(no_wzw(base), variant="pg_inf")
    c = rng.randrange(R_MOD)
    out["plus_g_equal_key"] = dict(random_args(rng, 7, 1, key=[c] * 11), wz=[5, 5, 0, 0], variant="plus_g")
    out["px_inf_all_infinity"] = dict(random_args(rng, 1, 0, key=[0] * 11), wires=[0] * 4, Z=0, t=[0] * 4, variant="px_inf")
    out["pg_inf_all_infinity"] = dict(no_wzw(random_args(rng, 1, 0, key=[0] * 11)), wires=[0] * 4, t=[0] * 4, variant="pg_inf")
    return out

