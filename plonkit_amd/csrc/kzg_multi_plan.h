// Many polynomials at several points with a two-element proof (kzg_multi.hip; Boneh-Drake-Fisch-Gabizon 2020): the host scalar algebra, as
// plain functions over HFr.  Host only, like prover_math.h and kzg_all_plan.h: no HIP, no environment, so a stand-alone program checks it
// against the Python-integer model (tests/host/kzg_multi_plan_check.cpp).  Prover and verifier call the same functions.
// NO COUNTERPART IN THE REFERENCE: bellman's kate_commitment opens at one point per call.
//
// f_0 .. f_{m-1}, points t_0 .. t_{p-1} (distinct), bit j of sets[i] = "f_i is opened at t_j" (S_i; T = all points).  With
//     Z_A(x) = prod_{a in A} (x - a),   w_ij = 1 / prod_{l in S_i, l != j} (t_j - t_l)   (the empty product is 1),
//     r_i = the polynomial of degree < |S_i| that agrees with f_i on S_i,   D_t[g] = (g - g(t)) / (x - t)
// the first quotient is
//     h = sum_i gamma^i (f_i - r_i) / Z_{S_i} = sum_j D_{t_j}[G_j],   G_j = sum_{i: j in S_i} gamma^i w_ij f_i
// because 1 / Z_{S_i} = sum_{j in S_i} w_ij / (x - t_j) (partial fractions) and (f_i - r_i)(t_j) = 0 on S_i, so each term
// w_ij (f_i - r_i) / (x - t_j) is the polynomial w_ij D_{t_j}[f_i] minus w_ij D_{t_j}[r_i], and sum_j w_ij D_{t_j}[r_i] =
// r_i / Z_{S_i} - sum_j w_ij r_i(t_j) / (x - t_j) = 0: the second sum is the partial-fraction expansion of r_i / Z_{S_i} itself
// (degree of r_i < |S_i|).  No interpolation, no long division.
// After the challenge u,  L = sum_i c_i (f_i - r_i(u)) - Z_T(u) h  with  c_i = gamma^i Z_{T \ S_i}(u)  vanishes at u, and the constant
// term of L does not reach L / (x - u) = D_u[sum_i c_i f_i - Z_T(u) h]: the same operator with one point and m + 1 polynomials.
#pragma once
#include <stdint.h>
#include "hostmath.h"

namespace plk {
namespace host {

constexpr uint32_t KM_MAX_POLYS = 64;                // polynomials of one quotient (plk_poly_quotient_multi_dev)
constexpr uint32_t KM_MAX_OPEN = 32;                 // polynomials of one opening: the second quotient takes them and h
constexpr uint32_t KM_MAX_POINTS = 8;
constexpr uint32_t KM_TILE = 2048, KM_THREADS = 256, KM_EPT = 8;     // the scan engine's block (poly.h): 8 coefficients per lane
constexpr uint32_t KM_LOG_THREADS = 8;
// per point, the constants of the three kernels (W domain): t^0 .. t^7 | t^(8 * 2^s), s < 8 | T = t^2048 | T^(per * 2^s), s < 8
constexpr uint32_t KM_C_POW = 0, KM_C_LANE = KM_EPT, KM_C_TILE = KM_C_LANE + KM_LOG_THREADS, KM_C_CHUNK = KM_C_TILE + 1, KM_CONSTS = KM_C_CHUNK + KM_LOG_THREADS;

inline HFr km_to_w(const HFr &c) { return c * HFr::from_u64(32); }       // W(c) = 2^261 c, in the external form 32 c (prover_math.h)

enum KmSetsVerdict : int { KM_SETS_OK = 0, KM_SETS_COUNTS, KM_SETS_DUPLICATE_POINT, KM_SETS_EMPTY, KM_SETS_BIT_ABOVE, KM_SETS_UNUSED_POINT };
inline const char *km_sets_words(int v) {
    switch (v) {
    case KM_SETS_OK: return "ok";
    case KM_SETS_COUNTS: return "the number of polynomials or of points is out of range";
    case KM_SETS_DUPLICATE_POINT: return "two of the points are equal";
    case KM_SETS_EMPTY: return "a polynomial is opened at no point (empty set)";
    case KM_SETS_BIT_ABOVE: return "a set names a point that does not exist";
    default: return "a point belongs to no set";
    }
}
// what both sides refuse about the sets, in this order
inline int km_check_sets(const HFr *points, uint32_t npoints, const uint32_t *sets, uint32_t count) {
    if (count == 0 || count > KM_MAX_OPEN || npoints == 0 || npoints > KM_MAX_POINTS) return KM_SETS_COUNTS;
    for (uint32_t a = 0; a < npoints; a++)
        for (uint32_t b = a + 1; b < npoints; b++) if (points[a] == points[b]) return KM_SETS_DUPLICATE_POINT;
    uint32_t used = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (sets[i] == 0) return KM_SETS_EMPTY;
        if (sets[i] >> npoints) return KM_SETS_BIT_ABOVE;
        used |= sets[i];
    }
    return used == (1u << npoints) - 1 ? KM_SETS_OK : KM_SETS_UNUSED_POINT;
}

// w[i * npoints + j] = w_ij for j in S_i, zero elsewhere.  ONE inversion for all of them: the denominators' running products, the
// inverse of the grand total, and the way back.
inline void km_weights(const HFr *points, uint32_t npoints, const uint32_t *sets, uint32_t count, HFr *w) {
    const uint32_t total = count * npoints;
    HFr prefix[KM_MAX_OPEN * KM_MAX_POINTS];                       // prefix[k] = d_0 .. d_{k-1}
    HFr run = HFr::one();
    for (uint32_t k = 0; k < total; k++) {                         // w[k] <- the denominator d_k (1 outside the set)
        const uint32_t i = k / npoints, j = k % npoints;
        HFr d = HFr::one();
        if ((sets[i] >> j) & 1)
            for (uint32_t l = 0; l < npoints; l++) if (l != j && ((sets[i] >> l) & 1)) d = d * (points[j] - points[l]);
        w[k] = d;
        prefix[k] = run;
        run = run * d;
    }
    HFr inv = run.inv();                                           // distinct points: no denominator is zero
    for (uint32_t k = total; k-- > 0;) {                           // inv = 1 / (d_0 .. d_k)
        const HFr d = w[k];
        w[k] = ((sets[k / npoints] >> (k % npoints)) & 1) ? inv * prefix[k] : HFr::zero();
        inv = inv * d;
    }
}

// m[i * npoints + j] = gamma^i w_ij: the matrix of the first quotient
inline void km_matrix(const HFr *w, const HFr &gamma, uint32_t count, uint32_t npoints, HFr *m) {
    HFr g = HFr::one();
    for (uint32_t i = 0; i < count; i++) {
        for (uint32_t j = 0; j < npoints; j++) m[i * npoints + j] = g * w[i * npoints + j];
        g = g * gamma;
    }
}

// Z_A(u) for the points named by `mask`
inline HFr km_z(const HFr *points, uint32_t npoints, uint32_t mask, const HFr &u) {
    HFr z = HFr::one();
    for (uint32_t j = 0; j < npoints; j++) if ((mask >> j) & 1) z = z * (u - points[j]);
    return z;
}

// c[i] = gamma^i Z_{T \ S_i}(u), *z_t = Z_T(u)
inline void km_c(const HFr *points, uint32_t npoints, const uint32_t *sets, uint32_t count, const HFr &gamma, const HFr &u, HFr *c, HFr *z_t) {
    const uint32_t all = (1u << npoints) - 1;
    HFr g = HFr::one();
    for (uint32_t i = 0; i < count; i++) { c[i] = g * km_z(points, npoints, all & ~sets[i], u); g = g * gamma; }
    *z_t = km_z(points, npoints, all, u);
}

// r_i(u) = sum_{j in S_i} y_ij w_ij prod_{l in S_i, l != j} (u - t_l): Lagrange's formula with the weights above, no division.
// w_row and y_row are row i of the count x npoints arrays; entries outside the set are not read.
inline HFr km_r_at(const HFr *points, uint32_t npoints, uint32_t mask, const HFr *w_row, const HFr *y_row, const HFr &u) {
    HFr r = HFr::zero();
    for (uint32_t j = 0; j < npoints; j++) {
        if (!((mask >> j) & 1)) continue;
        r = r + y_row[j] * w_row[j] * km_z(points, npoints, mask & ~(1u << j), u);
    }
    return r;
}

// the tiles of n coefficients, and how many of them one lane of the carry kernel walks
inline uint32_t km_tiles(uint64_t n) { return (uint32_t)((n + KM_TILE - 1) / KM_TILE); }
inline uint32_t km_chunk(uint32_t tiles) { return (tiles + KM_THREADS - 1) / KM_THREADS; }
// the KM_CONSTS constants of one point, in the W domain; 0^0 = 1, so t = 0 is an ordinary point
inline void km_point_constants(const HFr &t, uint32_t tiles, HFr *out) {
    HFr p = HFr::one();
    for (uint32_t e = 0; e < KM_EPT; e++) { out[KM_C_POW + e] = km_to_w(p); p = p * t; }
    for (uint32_t s = 0; s < KM_LOG_THREADS; s++) { out[KM_C_LANE + s] = km_to_w(p); p = p * p; }      // t^8, t^16 .. t^1024; then p = t^2048
    out[KM_C_TILE] = km_to_w(p);
    HFr q = p.pow_u64(km_chunk(tiles));
    for (uint32_t s = 0; s < KM_LOG_THREADS; s++) { out[KM_C_CHUNK + s] = km_to_w(q); q = q * q; }
}

}  // namespace host
}  // namespace plk
