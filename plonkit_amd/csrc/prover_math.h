// The host scalar algebra of the prover rounds (prover.hip): what the host computes between two challenges, as plain functions over
// HFr.  Host only, like msm_plan.h and ntt_dispatch.h: no HIP, no environment, so a stand-alone program checks it against the oracle
// (tests/host/prover_math_check.cpp).  Formulas: SURVEY.md Appendix A.4.
#pragma once
#include <stdint.h>
#include "hostmath.h"

namespace plk {
namespace host {

constexpr uint64_t NON_RESIDUES[4] = {1, 5, 7, 10};     // k_j (vk.bin stores 5, 7, 10); k_quotient (poly.hip) forms 5x, 7x, 10x by shifts

// ---- the W domain.  Vectors in HBM and scalars in the external form E carry the factor 2^256; a product of the 9 x 29-bit layer
// (field29_dev.h) is a * b * 2^-261, so a constant that meets such a product is handed over as c * 2^261 = W(c), on the host 32 * c in
// the external form (poly.h marks which arguments are W).  The other factors below bring a chain of several products back to 2^256 or
// 2^261 in one constant instead of converting anything per element.
constexpr uint64_t W_ONE = 32;                   // W(c) = 32 c
constexpr uint64_t W_FOUR_E_FACTORS = 1u << 25;  // 2^281: three E x E products leave 2^241, the fourth by this lands on 2^261 (k_perm_terms' fix);
                                                 //        the same for alpha against z times four 2^256 factors (QuotientArgs::alpha_pp)
constexpr uint64_t W_COSET_GEN = 7u << 5;        // W(7), the coset generator of the 4N domain
constexpr uint64_t W_LDE_SCALE = 1u << 10;       // a cached extension is stored with 2^261: as a factor of one product that itself removes 2^5
constexpr uint64_t W_LDE_SCALE_QM = 1u << 15;    // q_m with 2^266: it meets a product of two wires (2^251)
inline HFr to_w(const HFr &c) { return c * HFr::from_u64(W_ONE); }

// ---- round 3: the constants of the coset iNTT's combine step (k_icoset_combine) from i = omega_4: out[0] = i^-1, out[1 + c] = 7^(-N c) / 4
inline void icoset_constants_from(const HFr &omega4, uint32_t log_n, HFr out[5]) {
    const HFr gN_inv = HFr::from_u64(7).pow_u64(1ull << log_n).inv();
    out[0] = omega4.inv();
    out[1] = HFr::from_u64(4).inv();
    for (int c = 1; c < 4; c++) out[1 + c] = out[c] * gN_inv;
}

// ---- round 4
// the eleven evaluations of a proof in the order the device hands them back (and the transcript absorbs all but the order of the last three)
struct Evals {
    HFr v[11];
    const HFr *wz() const { return v; }              // a, b, c, d at z
    const HFr &w3zw() const { return v[4]; }         // d at z omega
    const HFr *sz() const { return v + 5; }          // sigma_0..2 at z
    const HFr &tz() const { return v[8]; }
    const HFr &zzw() const { return v[9]; }          // grand product at z omega
    const HFr &rz() const { return v[10]; }
};

// what the rounds need of the challenge z.  The three inversions (1/z, 1/(z omega), 1/(N (z - 1)) for L_0(z)) share one: the host inversion
// is what the GPU waits for between the rounds.
struct ZPoint { HFr z, zw, zN, z_inv, zw_inv, l0z; };
// nullptr, or the words of the refusal.  Any point of the domain is refused: every verifier refuses z^N = 1 (verify.cpp), so no proof is written
// for it.  Keccak gets there with probability N / r; a caller's transcript (plk_ctx_set_transcript) may be made to.
inline const char *challenge_point(const HFr &z, const HFr &omega, uint64_t N, ZPoint *out) {
    const HFr zw = z * omega, zN = z.pow_u64(N);
    if (z.is_zero()) return "challenge z = 0";
    const HFr l0_den = HFr::from_u64(N) * (z - HFr::one());
    if (l0_den.is_zero()) return "challenge z = 1";
    if (zN == HFr::one()) return "challenge z^N = 1";
    const HFr inv_all = (z * zw * l0_den).inv();
    out->z = z; out->zw = zw; out->zN = zN;
    out->z_inv = inv_all * zw * l0_den; out->zw_inv = inv_all * z * l0_den;
    out->l0z = (zN - HFr::one()) * (inv_all * z * zw);
    return nullptr;
}

// the two permutation factors of the linearisation: f_z multiplies z(x), f_sigma multiplies sigma_3(x)
inline void permutation_factors(const HFr &alpha, const HFr &beta, const HFr &gamma, const ZPoint &p, const Evals &e, HFr *fz, HFr *fs) {
    HFr a = alpha;
    for (int j = 0; j < 4; j++) a = a * (e.wz()[j] + beta * HFr::from_u64(NON_RESIDUES[j]) * p.z + gamma);
    *fz = a + alpha * alpha * p.l0z;
    HFr s = alpha * beta * e.zzw();
    for (int j = 0; j < 3; j++) s = s * (e.wz()[j] + beta * e.sz()[j] + gamma);
    *fs = s;
}

// r(x) = q_const + a q_a + b q_b + c q_c + d q_d + a b q_m + d(z omega) q_dnext + f_z z(x) - f_sigma sigma_3(x): the coefficients in that order
inline void linearisation_coefficients(const Evals &e, const HFr &fz, const HFr &fs, HFr out[9]) {
    const HFr *wz = e.wz();
    const HFr sc[9] = {HFr::one(), wz[0], wz[1], wz[2], wz[3], wz[0] * wz[1], e.w3zw(), fz, -fs};
    for (int k = 0; k < 9; k++) out[k] = sc[k];
}

// ---- round 5: opening at z of t_0 + z^N t_1 + z^2N t_2 + z^3N t_3 + v r + v^2..v^5 (a, b, c, d) + v^6..v^8 (sigma_0..2) — twelve coefficients —
// and at z omega of v^9 z(x) + v^10 d(x) — two
inline void opening_coefficients(const HFr &zN, const HFr &v, HFr at_z[12], HFr at_zw[2]) {
    HFr vp[11]; vp[0] = HFr::one();
    for (int k = 1; k <= 10; k++) vp[k] = vp[k - 1] * v;
    at_z[0] = HFr::one(); at_z[1] = zN; at_z[2] = zN * zN; at_z[3] = zN * zN * zN;
    for (int k = 1; k <= 8; k++) at_z[3 + k] = vp[k];
    at_zw[0] = vp[9]; at_zw[1] = vp[10];
}

}  // namespace host
}  // namespace plk
