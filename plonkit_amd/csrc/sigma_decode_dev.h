// sigma value -> cell: the inverse of k_sigma_from_index (poly.hip).  x = k_c * omega_N^i (k = 1, 5, 7, 10; N = 2^log_n) comes back as
// c << 30 | i, anything else as SIGMA_NOT_A_LABEL.  The group <omega_N> has 2-power order, so the discrete logarithm is exact and cheap
// (Pohlig-Hellman, one bit per step): x^N names the coset, then bit t of i is set iff (x / k_c * omega_N^-(i mod 2^t))^(N / 2^(t+1)) = -1.
// log_n + log_n (log_n - 1) / 2 squarings and 2 log_n + 3 products per value (the table powers are a product of two entries each).
//
// Acceptance does not rest on the logarithm: a value counts as decoded only if k_c * omega_N^i, recomputed exactly the way
// k_sigma_from_index computes it, equals x limb for limb.  0, a fifth coset, an element of order 2N and a non-canonical residue are all
// refused by that one comparison, whatever the steps before it made of them.
//
// __host__ __device__ over field_dev.h's Fr: the kernel (copycheck.hip) and the host program of the tests (tests/host/sigma_decode_kat.hip)
// build this same text.  The powers of omega_{2^28} come through two callables, pow_fwd(e) = omega^e and pow_inv(e) = omega^-e for
// e < 2^28: the two-level tables of the context on the device, whatever the host program likes.
#pragma once
#include "field_dev.h"

namespace plk {

constexpr uint32_t SIGMA_NOT_A_LABEL = 0xffffffffu;
constexpr uint32_t SIGMA_MAX_LOG_N = 26;                 // the largest setup: 4N = 2^28 is the 2-adicity of Fr
constexpr uint32_t SIGMA_ROOT_LOG = 28;                  // the tables hold powers of omega_{2^28}

// k[c] the coset representatives, k_inv[c] = 1 / k[c], k_pow_n[c] = k[c]^N for the N of the call (host-computed); Montgomery form
struct SigmaConsts { Fr k[4], k_inv[4], k_pow_n[4]; };

inline SigmaConsts sigma_consts(uint32_t log_n) {
    const uint64_t non_residues[4] = {1, 5, 7, 10};      // the k_j of prover.hip
    SigmaConsts C;
    for (int j = 0; j < 4; j++) {
        const Fr k = from_u64<FrParams>(non_residues[j]);
        Fr kn = k;
        for (uint32_t s = 0; s < log_n; s++) kn = sqr(kn);
        C.k[j] = k; C.k_inv[j] = inv(k); C.k_pow_n[j] = kn;
    }
    return C;
}

template <class PowFwd, class PowInv>
PLK_HD uint32_t sigma_decode(const Fr &x, uint32_t log_n, const SigmaConsts &C, const PowFwd &pow_fwd, const PowInv &pow_inv) {
    // coset: x^N against the four k_c^N (they differ: k_c / k_c' is no N-th root of unity, or the cosets would meet)
    Fr xn = x;
    for (uint32_t s = 0; s < log_n; s++) xn = sqr(xn);
    uint32_t c = 4;
    Fr y = x, kc = C.k[0];
    if (xn == C.k_pow_n[0]) c = 0;                       // k_0 = 1: y = x
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (c == 4 && xn == C.k_pow_n[j]) { c = (uint32_t)j; y = mul(x, C.k_inv[j]); kc = C.k[j]; }
    if (c == 4) return SIGMA_NOT_A_LABEL;
    // row: y lies in <omega_N> now (y^N = 1).  Before step t its order divides N / 2^t.
    const Fr one = Fr::one();
    const uint32_t up = SIGMA_ROOT_LOG - log_n;          // omega_N^e = omega_{2^28}^(e << up)
    uint32_t i = 0;
    for (uint32_t t = 0; t < log_n; t++) {
        Fr z = y;
        for (uint32_t s = t + 1; s < log_n; s++) z = sqr(z);                 // y^(N / 2^(t+1)): 1 or -1
        const bool bit = z != one;
        const Fr cleared = mul(y, pow_inv((1u << t) << up));                 // (computed on every lane: the wave does not split here)
        if (bit) { y = cleared; i |= 1u << t; }
    }
    // the acceptance rule: the label of (c, i) as k_sigma_from_index writes it
    const Fr w = pow_fwd(i << up);
    const Fr label = c == 0 ? w : mul(w, kc);
    return label == x ? (c << 30 | i) : SIGMA_NOT_A_LABEL;
}

}  // namespace plk
