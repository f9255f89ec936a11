// The scalar front of one multi-point opening as host + device code (kzg_multi_verify.hip: one opening per lane): the checks
// plk_kzg_verify_multi (kzg_multi.hip) makes of an opening's own data, and the count + 3 scalars its group arithmetic multiplies by,
//     c_0 .. c_{count-1}   |   -sum_i c_i r_i(u)   |   -Z_T(u)   |   u            for   C_0 .. C_{count-1}, G, W, W'.
// NO COUNTERPART IN THE REFERENCE (kate_commitment opens at one point per call).  It restates km_weights, km_c and km_r_at
// (kzg_multi_plan.h) so that a lane never holds a count x npoints array:
//   - the pairs t_j - t_l, j < l (at most 28), are inverted together by ONE fr_inv_call; their running products, and then the inverses,
//     live in the opening's slot of the pass buffer (`run`, `stride` elements apart: the kernel lays the slots out lane-major);
//   - w_ij = prod_{l in S_i, l != j} 1 / (t_j - t_l) is a product of those inverses, negated once for every l < j; it is folded
//     straight into the term y_ij w_ij prod_{l in S_i, l != j} (u - t_l) of r_i(u);
//   - points, evaluations and inverses are read again from memory where they are needed: nothing indexed sits in registers.
// A scalar mod r has one canonical form, so the words are km_c's and km_r_at's whatever the order of the products.
// Everything is __host__ __device__ (tests/host/kzg_multi_verify_check.hip runs the same text on the CPU against kzg_multi_plan.h and
// the Python-integer model); field products go through FRM, one out-of-line copy on the device (verify_front_dev.h).
#pragma once
#include "fq12_dev.h"
#include "verify_front_dev.h"
#include "kzg_multi_verify_plan.h"

namespace plk {

// the batch's shape, a kernel argument: one protocol, many proofs
struct KmvShape {
    uint32_t count, npoints;
    uint32_t sets[host::KMV_MAX_OPEN];
};

#if defined(__HIP_DEVICE_COMPILE__)
#define KMV_LD(p) load_fp(p)
#define KMV_ST(p, v) store_fp((p), (v))
#define KMV_LD_POINT(p) load_affine(p)
#else
#define KMV_LD(p) (*(p))
#define KMV_ST(p, v) (*(p) = (v))
#define KMV_LD_POINT(p) (*(p))
#endif

PLK_HD bool kmv_fr_below_modulus(const Fr &v) {
    uint64_t br = 0;
    for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)v.l[i] - FrParams::P[i] - br; br = (d >> 32) & 1; }
    return br != 0;
}
PLK_HD_CALL bool kmv_point_ok(const G1Affine &p) {                    // (0, 0) is infinity, a legal commitment, W and W'
    return fq_below_modulus(p.x) && fq_below_modulus(p.y) && fq_on_curve(p.x, p.y);
}

// what plk_kzg_verify_multi refuses with PLK_ERR_ARG about the opening's own data, the equality of two points apart (kmv_invert_pairs):
// a point off the curve, a coordinate >= q, gamma, u, a point or an evaluation INSIDE its set >= r.  Evaluations outside a set are not read.
PLK_HD bool kmv_well_formed(const KmvShape &S, const G1Affine *cm, const Fr *pts, const Fr *ev, const Fr *gamma, const Fr *u, const G1Affine *proofs) {
    if (!kmv_fr_below_modulus(KMV_LD(gamma)) || !kmv_fr_below_modulus(KMV_LD(u))) return false;
#pragma unroll 1
    for (uint32_t j = 0; j < S.npoints; j++) if (!kmv_fr_below_modulus(KMV_LD(pts + j))) return false;
#pragma unroll 1
    for (uint32_t k = 0; k < 2; k++) if (!kmv_point_ok(KMV_LD_POINT(proofs + k))) return false;
#pragma unroll 1
    for (uint32_t i = 0; i < S.count; i++) {
        if (!kmv_point_ok(KMV_LD_POINT(cm + i))) return false;
#pragma unroll 1
        for (uint32_t j = 0; j < S.npoints; j++)
            if (((S.sets[i] >> j) & 1) && !kmv_fr_below_modulus(KMV_LD(ev + i * S.npoints + j))) return false;
    }
    return true;
}

// run[kmv_pair(j, l) * stride] = 1 / (t_j - t_l) for j < l; false when two points are equal (nothing useful is left in run then)
PLK_HD bool kmv_invert_pairs(const Fr *pts, uint32_t npoints, Fr *run, size_t stride) {
    if (npoints < 2) return true;
    Fr total = Fr::one();
    uint32_t k = 0;
#pragma unroll 1
    for (uint32_t j = 0; j + 1 < npoints; j++) {
        const Fr tj = KMV_LD(pts + j);
#pragma unroll 1
        for (uint32_t l = j + 1; l < npoints; l++, k++) {
            const Fr d = sub(tj, KMV_LD(pts + l));
            if (d.is_zero()) return false;
            KMV_ST(run + k * stride, total);                          // d_0 .. d_{k-1}
            total = FRM(total, d);
        }
    }
    Fr inv = fr_inv_call(total);                                      // 1 / (d_0 .. d_k) while walking back
#pragma unroll 1
    for (uint32_t j = npoints - 1; j-- > 0;) {
        const Fr tj = KMV_LD(pts + j);
#pragma unroll 1
        for (uint32_t l = npoints - 1; l > j; l--) {
            k--;
            const Fr d = sub(tj, KMV_LD(pts + l));
            KMV_ST(run + k * stride, FRM(inv, KMV_LD(run + k * stride)));
            inv = FRM(inv, d);
        }
    }
    return true;
}

// y_ij w_ij prod_{l in S_i, l != j} (u - t_l): one term of Lagrange's formula for r_i(u), with the inverses of kmv_invert_pairs
PLK_HD_CALL Fr kmv_lagrange_term(const Fr *pts, uint32_t npoints, uint32_t mask, uint32_t j, const Fr &y, const Fr &u, const Fr *run, size_t stride) {
    Fr t = y;
    bool flip = false;
#pragma unroll 1
    for (uint32_t l = 0; l < npoints; l++) {
        if (l == j || !((mask >> l) & 1)) continue;
        t = FRM(t, sub(u, KMV_LD(pts + l)));
        t = FRM(t, KMV_LD(run + (size_t)(l < j ? host::kmv_pair(l, j, npoints) : host::kmv_pair(j, l, npoints)) * stride));
        flip ^= l < j;                                                // 1 / (t_j - t_l) = -1 / (t_l - t_j)
    }
    return flip ? neg(t) : t;
}

// State 1: the opening goes on to the group arithmetic with sc[0 .. count + 3).  State 2: malformed, the scalars are zero.
// cm: count points, pts: npoints scalars, ev: count x npoints scalars, proofs: W, W'; run: kmv_pairs(npoints) elements, `stride` apart.
PLK_HD uint32_t kmv_front(const KmvShape &S, const G1Affine *cm, const Fr *pts, const Fr *ev, const Fr *gamma_p, const Fr *u_p, const G1Affine *proofs,
                          Fr *run, size_t stride, Fr *sc) {
    const uint32_t m = S.count, p = S.npoints;
    if (!kmv_well_formed(S, cm, pts, ev, gamma_p, u_p, proofs) || !kmv_invert_pairs(pts, p, run, stride)) {
#pragma unroll 1
        for (uint32_t t = 0; t < m + 3; t++) KMV_ST(sc + t, Fr::zero());
        return host::KMV_STATE_MALFORMED;
    }
    const Fr gamma = KMV_LD(gamma_p), u = KMV_LD(u_p);
    Fr g = Fr::one(), sum = Fr::zero();                               // gamma^i, sum_i c_i r_i(u)
#pragma unroll 1
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t mask = S.sets[i];
        Fr c = g, r = Fr::zero();                                     // c_i = gamma^i Z_{T \ S_i}(u)
#pragma unroll 1
        for (uint32_t j = 0; j < p; j++) {
            if ((mask >> j) & 1) r = add(r, kmv_lagrange_term(pts, p, mask, j, KMV_LD(ev + i * p + j), u, run, stride));
            else c = FRM(c, sub(u, KMV_LD(pts + j)));
        }
        sum = add(sum, FRM(c, r));
        KMV_ST(sc + i, c);
        g = FRM(g, gamma);
    }
    Fr z_t = Fr::one();                                               // Z_T(u)
#pragma unroll 1
    for (uint32_t j = 0; j < p; j++) z_t = FRM(z_t, sub(u, KMV_LD(pts + j)));
    KMV_ST(sc + m, neg(sum));
    KMV_ST(sc + m + 1, neg(z_t));
    KMV_ST(sc + m + 2, u);
    return host::KMV_STATE_GOES_ON;
}

}  // namespace plk
