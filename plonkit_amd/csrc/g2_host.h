// Host arithmetic on the twist y^2 = x^3 + 3 / xi over Fq2, for the things the pairing code does not do: the subgroup check [r]Q = O
// (keycheck.hip) and s * Q of a key update (srs_update.hip).  Jacobian coordinates, the formulas of hostmath.h's jac_double / jac_add
// (a = 0).  Infinity is z = 0.  The twist has odd order, so a doubling never meets y = 0.
#pragma once
#include "pairing.h"

namespace plk {
namespace host {

struct G2Jac { Fq2 x, y, z; };
inline G2Jac g2_jac_inf() { return G2Jac{Fq2::one(), Fq2::one(), Fq2::zero()}; }
inline Fq2 twice(const Fq2 &a) { return a + a; }
inline G2Jac g2_double(const G2Jac &p) {
    if (p.z.is_zero()) return p;
    const Fq2 A = p.x.sqr(), B = p.y.sqr(), C = B.sqr();
    const Fq2 D = twice((p.x + B).sqr() - A - C), E = twice(A) + A;
    G2Jac r;
    r.x = E.sqr() - twice(D);
    r.z = twice(p.y * p.z);
    r.y = E * (D - r.x) - twice(twice(twice(C)));
    return r;
}
inline G2Jac g2_add(const G2Jac &p, const G2Jac &q) {
    if (q.z.is_zero()) return p;
    if (p.z.is_zero()) return q;
    const Fq2 z1z1 = p.z.sqr(), z2z2 = q.z.sqr();
    const Fq2 u1 = p.x * z2z2, u2 = q.x * z1z1, s1 = p.y * q.z * z2z2, s2 = q.y * p.z * z1z1;
    if (u1 == u2) return (s1 == s2) ? g2_double(p) : g2_jac_inf();
    const Fq2 h = u2 - u1, i = twice(h).sqr(), j = h * i, rr = twice(s2 - s1), v = u1 * i;
    G2Jac r;
    r.x = rr.sqr() - j - twice(v);
    r.y = rr * (v - r.x) - twice(s1 * j);
    r.z = ((p.z + q.z).sqr() - z1z1 - z2z2) * h;
    return r;
}
// k * q, k canonical little-endian limbs below 2^254; q on the twist (infinity allowed)
inline G2Jac g2_mul(const G2Affine &q, const uint64_t k[4]) {
    G2Jac acc = g2_jac_inf();
    if (q.inf) return acc;
    const G2Jac base{q.x, q.y, Fq2::one()};
    for (int i = 253; i >= 0; i--) {
        acc = g2_double(acc);
        if ((k[i >> 6] >> (i & 63)) & 1) acc = g2_add(acc, base);
    }
    return acc;
}
inline bool g2_in_subgroup(const G2Affine &q) {                 // q on the twist and not infinity; r < 2^254
    return g2_mul(q, FrP::P).z.is_zero();
}
inline G2Affine g2_to_affine(const G2Jac &p) {
    if (p.z.is_zero()) return G2Affine{Fq2::zero(), Fq2::zero(), true};
    const Fq2 zi = p.z.inv(), zi2 = zi.sqr();
    return G2Affine{p.x * zi2, p.y * zi2 * zi, false};
}
// the inverse of g2_from_bytes: x.c1 || x.c0 || y.c1 || y.c0, infinity as 0x40 00..00
inline void g2_to_bytes(const G2Affine &q, uint8_t out[128]) {
    if (q.inf) { for (int i = 0; i < 128; i++) out[i] = 0; out[0] = 0x40; return; }
    q.x.c1.to_be_bytes(out); q.x.c0.to_be_bytes(out + 32); q.y.c1.to_be_bytes(out + 64); q.y.c0.to_be_bytes(out + 96);
}

}  // namespace host
}  // namespace plk
