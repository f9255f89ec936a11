// Carry-free 9 x 29-bit-limb arithmetic for the VALU-bound kernels (NTT butterflies, MSM).
//
// Why: on gfx950 every carry-producing VALU op (v_add_co/v_addc, 64-bit adds) costs the same
// ~4.2 cycles per wave as a v_mad_u64_u32, while plain v_add_u32/v_and/v_lshr cost ~2.25
// (profiles/r01_ubench_int2.txt).  The 8 x 32-bit CIOS product of field_dev.h spends 128 mads + 130
// 64-bit adds + 275 moves per product (~1600 cycles per wave).  With 29-bit limbs a column of
// 18 partial products fits a 64-bit accumulator without any carry handling: 162 mads + a short
// normalisation (~900 cycles), and additions/subtractions become 9 plain 32-bit ops.
//
// Representation W: value = sum l[i] * 2^(29 i), 9 limbs, capacity 2^261 = ~170 p.
// Montgomery radix inside this layer is R' = 2^261 (nine 29-bit reduction steps):
//     mulw(a, b) = a * b * 2^-261 mod p,   result < a*b/2^261 + p   (not fully reduced)
// p / 2^261 = 0.0059, so sums of several un-reduced values can be multiplied again without any
// conditional subtraction ("lazy reduction"); bounds are tracked per call site.
// Data in HBM keeps the library's external form (8 x u32, R = 2^256): the NTT is linear, so it can
// run W arithmetic on the raw 256-bit values as long as the twiddle CONSTANTS are in the 2^261
// domain; the MSM keeps its resident SRS and its accumulators in the 2^261 domain and converts
// at the boundary.  No MFMA: these are 29x29->58-bit integer multiply-adds on the VALU.
#pragma once
#include "field_dev.h"
#include <type_traits>
#include <utility>

namespace plk {

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N-1>{}) — `#pragma unroll` is only a
// request, and a loop the compiler leaves rolled puts the register arrays it indexes into scratch memory
template <int... J, class F> __device__ __forceinline__ void static_for_impl(std::integer_sequence<int, J...>, F &&f) { (f(std::integral_constant<int, J>{}), ...); }
template <int N, class F> __device__ __forceinline__ void static_for(F &&f) { static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F &&>(f)); }

constexpr uint32_t M29 = (1u << 29) - 1;
constexpr uint32_t MULW_A_LIMB_MAX = 3280000000u;          // largest limb of mulw's LEFT operand (the columns then just fit: asserted at mont_scan)

struct FrW {
    static constexpr uint32_t P29[9] = {0x10000001u, 0x1f0fac9fu, 0x0e5c2450u, 0x07d090f3u, 0x1585d283u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu};
    static constexpr uint32_t INV29 = 0x0fffffffu;                   // -p^-1 mod 2^29
    static constexpr uint32_t PINV0 = 0x10000001u;                   //  p^-1 mod 2^29
    static constexpr uint32_t ONE_W[9] = {0x0fffff57u, 0x1ea70ab4u, 0x052c068bu, 0x17504f49u, 0x0aa8075bu, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u};
    static constexpr uint32_t W_FROM_S[9] = {0x0fffead7u, 0x1d5444f4u, 0x04438aa5u, 0x03b4d096u, 0x134c84dau, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u};
    static constexpr uint32_t S_FROM_W[9] = {0x0ffffffbu, 0x04b1a0e2u, 0x18334a6bu, 0x18ed2b3eu, 0x1462e36fu, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u};
    static constexpr uint32_t PAD2[9] = {0x80000002u, 0x9e1f593bu, 0x9cb8489du, 0x8fa121e2u, 0x8b0ba502u, 0x85b6817du, 0x814dc27eu, 0x9cb84c64u, 0x0060c898u};
    static constexpr uint32_t PAD4[9] = {0x80000004u, 0x9c3eb27au, 0x9970913fu, 0x9f4243c9u, 0x96174a08u, 0x8b6d02feu, 0x829b8500u, 0x997098ccu, 0x00c19135u};
    static constexpr uint32_t PAD6[9] = {0x80000006u, 0x9a5e0bb9u, 0x9628d9e1u, 0x8ee365b0u, 0x8122ef0fu, 0x91238480u, 0x83e94782u, 0x9628e534u, 0x012259d2u};
    static constexpr uint32_t PAD8[9] = {0x80000008u, 0x987d64f8u, 0x92e12283u, 0x9e848797u, 0x8c2e9415u, 0x96da0601u, 0x85370a04u, 0x92e1319cu, 0x0183226fu};
    // 2^-29 mod p for the folded digits (below, "THE FOLD"); (p + 1) / 2 with no multiple of p added: no form of this field folds yet, and of the
    // representatives below 4p (the value rule) this one has the smallest worst columns (0.65 * 2^64 for normalised products)
    static constexpr uint32_t FOLDC[9] = {0x18f05361u, 0x012bb1feu, 0x0f5d8135u, 0x1e6275f6u, 0x07e7a880u, 0x10c6bf1fu, 0x11f74a6cu, 0x06fdaecbu, 0x00183227u};
};

struct FqW {
    static constexpr uint32_t P29[9] = {0x187cfd47u, 0x010460b6u, 0x1c72a34fu, 0x02d522d0u, 0x1585d978u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu};
    static constexpr uint32_t INV29 = 0x04866389u;
    static constexpr uint32_t PINV0 = 0x1b799c77u;
    static constexpr uint32_t ONE_W[9] = {0x157ccc21u, 0x141c2758u, 0x185230d3u, 0x014c0419u, 0x0aa36fb9u, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u};
    static constexpr uint32_t W_FROM_S[9] = {0x13349ca1u, 0x1a5d84a8u, 0x0a3e5cacu, 0x100249e0u, 0x12b951e8u, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u};
    static constexpr uint32_t S_FROM_W[9] = {0x058f0d9du, 0x1aea1c6eu, 0x11c2cf74u, 0x11d651ebu, 0x1462c0a7u, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u};
    static constexpr uint32_t PAD2[9] = {0x90f9fa8eu, 0x8208c169u, 0x98e5469au, 0x85aa459du, 0x8b0bb2ecu, 0x85b6817du, 0x814dc27eu, 0x9cb84c64u, 0x0060c898u};
    static constexpr uint32_t PAD4[9] = {0x81f3f51cu, 0x841182d7u, 0x91ca8d38u, 0x8b548b3fu, 0x961765dcu, 0x8b6d02feu, 0x829b8500u, 0x997098ccu, 0x00c19135u};
    static constexpr uint32_t PAD6[9] = {0x92edefaau, 0x861a4444u, 0x8aafd3d6u, 0x90fed0e1u, 0x812318ccu, 0x91238480u, 0x83e94782u, 0x9628e534u, 0x012259d2u};
    static constexpr uint32_t PAD8[9] = {0x83e7ea38u, 0x882305b2u, 0x83951a74u, 0x96a91683u, 0x8c2ecbbcu, 0x96da0601u, 0x85370a04u, 0x92e1319cu, 0x0183226fu};
    // 2p and 6p with the lower limbs biased by 2^29 only: enough to subtract a NORMALISED value limb by limb (limbs < 2^29), and the
    // difference keeps limbs below 2^30 (+ 2^29 with a normalised term added) — small enough to enter mul2addw as a right operand as
    // it stands (xyzzw_add_mixed_flag; the 2^31 bias of the pads above is what a subtrahend with limbs up to 2^30 needs)
    static constexpr uint32_t PAD2N[9] = {0x30f9fa8eu, 0x2208c16cu, 0x38e5469du, 0x25aa45a0u, 0x2b0bb2efu, 0x25b68180u, 0x214dc281u, 0x3cb84c67u, 0x0060c89bu};
    static constexpr uint32_t PAD6N[9] = {0x32edefaau, 0x261a4447u, 0x2aafd3d9u, 0x30fed0e4u, 0x212318cfu, 0x31238483u, 0x23e94785u, 0x3628e537u, 0x012259d5u};
    // 2^-29 mod p + 2p = 2.1414 p for the folded digits (below, "THE FOLD").  Of the 170 representatives below 2^261 this one has by far the smallest
    // limbs (they sum to 1.03e9 against 1.62e9 for p's) and the smallest worst column in every form that folds: 0.426 * 2^64 for normalised products
    // and squarings (0.501 unfolded), 0.848 for the +-y chain with its addend (0.923), 0.771 for the fused Y3 (0.845), 0.372 for tw2 (0.425), 0.181
    // for make_tw2_a (0.211); the next best representative (+ 100p) reaches 0.919 and adds fifty times as much to a result.
    static constexpr uint32_t FOLDC[9] = {0x0872952du, 0x0808854au, 0x065124e0u, 0x029b9885u, 0x03f6b850u, 0x148e9764u, 0x02b3e954u, 0x0843f777u, 0x0067a061u};
};

template <class WP>
struct W9 {
    uint32_t l[9];
};

template <class WP> PLK_HD W9<WP> w_zero() { W9<WP> r; for (int i = 0; i < 9; i++) r.l[i] = 0; return r; }
template <class WP> PLK_HD W9<WP> w_one() { W9<WP> r; for (int i = 0; i < 9; i++) r.l[i] = WP::ONE_W[i]; return r; }
template <class WP> PLK_HD W9<WP> w_from_s_const() { W9<WP> r; for (int i = 0; i < 9; i++) r.l[i] = WP::W_FROM_S[i]; return r; }
template <class WP> PLK_HD W9<WP> s_from_w_const() { W9<WP> r; for (int i = 0; i < 9; i++) r.l[i] = WP::S_FROM_W[i]; return r; }
template <class WP> PLK_HD bool w_all_zero(const W9<WP> &a) { uint32_t o = 0; for (int i = 0; i < 9; i++) o |= a.l[i]; return o == 0; }

// 8 x u32 packed -> 9 x 29 (no arithmetic; the 256-bit integer is re-sliced)
template <class WP, class PR>
PLK_HD W9<WP> unpack(const Fp<PR> &a) {
    W9<WP> r;
    const uint32_t *w = a.l;
    r.l[0] = w[0] & M29;
    r.l[1] = ((w[0] >> 29) | (w[1] << 3)) & M29;
    r.l[2] = ((w[1] >> 26) | (w[2] << 6)) & M29;
    r.l[3] = ((w[2] >> 23) | (w[3] << 9)) & M29;
    r.l[4] = ((w[3] >> 20) | (w[4] << 12)) & M29;
    r.l[5] = ((w[4] >> 17) | (w[5] << 15)) & M29;
    r.l[6] = ((w[5] >> 14) | (w[6] << 18)) & M29;
    r.l[7] = ((w[6] >> 11) | (w[7] << 21)) & M29;
    r.l[8] = w[7] >> 8;
    return r;
}

// normalised limbs, value < 2^256  ->  8 x u32
template <class PR, class WP>
PLK_HD Fp<PR> pack(const W9<WP> &a) {
    Fp<PR> r;
    const uint32_t *l = a.l;
    r.l[0] = l[0] | (l[1] << 29);
    r.l[1] = (l[1] >> 3) | (l[2] << 26);
    r.l[2] = (l[2] >> 6) | (l[3] << 23);
    r.l[3] = (l[3] >> 9) | (l[4] << 20);
    r.l[4] = (l[4] >> 12) | (l[5] << 17);
    r.l[5] = (l[5] >> 15) | (l[6] << 14);
    r.l[6] = (l[6] >> 18) | (l[7] << 11);
    r.l[7] = (l[7] >> 21) | (l[8] << 8);
    return r;
}

// carry propagation: limbs (<= 2^32 - 8: a carry is at most 7 and limb + carry must fit 32 bits; total value < 2^261) -> limbs < 2^29.
// (The lazy butterflies of ntt.hip feed in x + PAD2 - y + c, limbs < 3.74e9.)  Pinned at 2^32 - 8 by tests/test_arith_kat_host.py.
template <class WP>
PLK_HD W9<WP> normw(const W9<WP> &a) {
    W9<WP> r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { uint32_t s = a.l[i] + c; r.l[i] = s & M29; c = s >> 29; }
    r.l[8] = a.l[8] + c;
    return r;
}

// limb-wise sum, no carry handling (limbs grow by one bit)
template <class WP>
PLK_HD W9<WP> addw(const W9<WP> &a, const W9<WP> &b) {
    W9<WP> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = a.l[i] + b.l[i];
    return r;
}

// a - b + k*p, where k*p is held with its lower limbs biased by 2^31 (PADk) so that no limb goes
// negative; b limbs < 2^30, b < k*p.  Result normalised, value < a + k*p.
template <class WP, int K> PLK_HD W9<WP> sub_pad(const W9<WP> &a, const W9<WP> &b) {
    static_assert(K == 2 || K == 4 || K == 6, "sub_pad: no pad for this multiple of p");
    W9<WP> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = a.l[i] + (K == 2 ? WP::PAD2[i] : K == 4 ? WP::PAD4[i] : WP::PAD6[i]) - b.l[i];
    return normw(r);
}
template <class WP> PLK_HD W9<WP> sub2(const W9<WP> &a, const W9<WP> &b) { return sub_pad<WP, 2>(a, b); }
template <class WP> PLK_HD W9<WP> sub4(const W9<WP> &a, const W9<WP> &b) { return sub_pad<WP, 4>(a, b); }
template <class WP> PLK_HD W9<WP> sub6(const W9<WP> &a, const W9<WP> &b) { return sub_pad<WP, 6>(a, b); }
template <class WP> PLK_HD W9<WP> neg2(const W9<WP> &a) { return sub_pad<WP, 2>(w_zero<WP>(), a); }   // 2p - a for a < 2p (negation)
template <class WP> PLK_HD W9<WP> addn(const W9<WP> &a, const W9<WP> &b) { return normw(addw(a, b)); }

// ---- Montgomery product, radix 2^29, R' = 2^261 — PRODUCT SCANNING.  The 17 columns of a*b + m*p are summed one after the other in
// ONE 64-bit accumulator per chain; the carry of column k (acc >> 29) is the addend of the first multiply-add of column k+1, so no 64-bit
// addition is ever issued (operand scanning paid one v_lshl_add_u64 per row plus eight in the final normalisation: 58 non-mad
// instructions per product against 42 here).  Columns 0..8 give the digit m_k and the carry, columns 9..16 an output limb.
// The scan is written ONCE (mont_scan); every form below is an instantiation of it:
//   - one chain or two in lockstep: the multiply-adds of two accumulator chains alternate one by one, so that no v_mad_u64_u32 reads the
//     result of the one issued just before it (on gfx950 that costs a wait state: the compiler puts an s_nop between every pair of a
//     single chain);
//   - an OPERAND HALF per chain, which adds a column's a*b terms: T products (Products), a squaring (Squaring), a shift (Shift5);
//   - LZ, the set of digits m_0..m_7 left UNMASKED (bit k for m_k; bit 8 and above are ignored; 0 is the masked form);
//   - an optional 9-limb ADDEND that joins the high columns.
// PLK_CHAIN pins the association: left alone, the compiler sums a column apart from the carry and joins the two with the very addition
// this form exists to avoid.
// LAZY DIGITS.  A column's digit is m_k = ((uint32_t)acc * INV29) & M29, but any m~_k = m_k (mod 2^29) clears the column's low 29 bits just
// as well: (a*b + m~*p) / 2^261 stays an exact integer congruent to a*b*2^-261, and the `& M29` of that digit, one VALU instruction, is not
// issued (the additions the MSM prices by the instructions they issue: xyzzw_add_mixed_flag, xyzzw_add_pairs).  Two things depend on the
// mask, and both are kept:
//   - the VALUE of the result.  Digit 8 is always masked: with m~_0..m~_7 < 2^32 and m~_8 < 2^29, m~ = sum m~_k 2^(29 k) < 2^261 + 2^235, and
//     m~ = m (mod 2^261), so m~ is m or m + 2^261: the result is the masked form's or that plus p EXACTLY, and it is below the masked form's
//     bound + 2^-26 p.  Every value bound of ec29_dev.h has more slack than that.  Output limbs are normalised as before.
//   - the 64-bit COLUMN.  Every instantiation, masked or lazy, evaluates its exact worst case at compile time (lazy_col_bound: every limb of
//     every operand at its DECLARED bound, a Limbs9 per operand; every unmasked digit at 2^32 - 1 and every masked one at 2^29 - 1 against
//     the actual limbs of p; the addend where there is one; the carry the worst column before it really leaves) and a static_assert
//     requires every column below 2^64: a form that does not fit does not compile.  The declared bounds are the caller's promise, checked
//     on the host at exactly those limbs (tests/host/field29_check.hip, field29_addend_check.hip, field29_lazy_digits_check.hip).
// THE FOLD.  A Montgomery digit costs one v_mul_lo_u32, as much as a multiply-add, only to find the multiple of p that clears the column.  The same
// division by 2^29 needs no such product: with C = 2^-29 (mod p) (WP::FOLDC, nine limbs below 2^29) and L the low word of column k's accumulator,
// L 2^(29 k) = L C 2^(29 (k + 1)) (mod p), so the column is emptied by REMOVING L and adding L * C[j] to columns k + 1 + j, j = 0..8: nine multiply-adds,
// as many as m_k * p takes (the term in column k goes, one in column k + 9 comes).  FOLD is the set of digits treated so (bit k for digit k; 0 is the
// text above).  For a folded digit: digit(k) is the accumulator's low register as it stands where the digit is also in LZ - no product, no mask,
// L < 2^32, and the carry into column k + 1 is (acc - L) / 2^29 = (acc >> 32) << 3 - and acc & M29 with the usual acc >> 29 otherwise; mp0(k) is
// nothing; column k' > k takes m[k] * FOLDC[k' - k - 1] where it took m[k] * P29[k' - k].
//   - the VALUE.  L * C is not small as m * p / 2^29 < p is: digit k of D adds L C / 2^(29 (D - 1 - k)) to the result.  So only a PREFIX 0..f-1 with
//     f <= D - 2 folds: every folded digit is then divided by at least 2^58 and the set adds less than 2^32 C / 2^58 (1 + 2^-28) = (C / p) 2^-26 p
//     (1 + 2^-28); the last two digits stay Montgomery digits (the last one masked) and bound the result as before.  fold_value_ok requires the
//     prefix and (C / p) 2^-26 (1 + 2^-28) <= 2^-24 by static_assert in every form: a set with digit D - 2 or D - 1, or with a gap, does not compile.
//     With FqW::FOLDC = 2.1414 p a folded reduction's result is below the lazy form's bound + 2.15 * 2^-26 p.
//   - the COLUMN.  lazy_col_bound, tw2_col_bound and tw2a_col_bound take the folded digits (2^32 - 1 unmasked, 2^29 - 1 masked) against FOLDC's limbs
//     one column up, and the carry as acc >> 29, which (acc >> 32) << 3 never exceeds; the same static_assert refuses a form that does not fit.
#if defined(__HIP_DEVICE_COMPILE__)
#define PLK_CHAIN(acc) asm("" : "+v"(acc))
// (the addend enters as a multiply-add by a one the compiler cannot see: the plain 64-bit addition it would otherwise form wants the
//  addend widened to a register pair, one extra move per limb)
#define PLK_ADDEND(acc, x) { uint32_t one_ = 1; asm("" : "+s"(one_)); (acc) += (uint64_t)(x) * one_; }
// (the carry out of a folded unmasked digit, (acc >> 32) << 3, as ONE instruction: the high register times an eight the compiler cannot see, a
//  multiply-add onto zero that costs what the v_lshrrev_b64 of a Montgomery digit costs; written as shifts it becomes that shift and two masks)
#define PLK_FOLD_CARRY(acc) { uint32_t eight_ = 8; asm("" : "+s"(eight_)); (acc) = (uint64_t)(uint32_t)((acc) >> 32) * eight_; }
#else
#define PLK_CHAIN(acc) do { } while (0)
#define PLK_ADDEND(acc, x) { (acc) += (uint64_t)(x); }
#define PLK_FOLD_CARRY(acc) { (acc) = (uint64_t)(uint32_t)((acc) >> 32) << 3; }
#endif
struct Limbs9 { uint32_t l[9]; };                              // per-limb upper bounds of an operand (inclusive)
constexpr Limbs9 lb_uniform(uint32_t v) { return Limbs9{{v, v, v, v, v, v, v, v, v}}; }
constexpr Limbs9 lb_of(const uint32_t (&a)[9]) { return Limbs9{{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]}}; }
constexpr Limbs9 lb_plus(const Limbs9 &a, uint32_t v) { Limbs9 r{}; for (int i = 0; i < 9; i++) r.l[i] = a.l[i] + v; return r; }
constexpr bool lb_below(const Limbs9 &a, uint32_t v) { for (int i = 0; i < 9; i++) if (a.l[i] >= v) return false; return true; }
constexpr Limbs9 lb_max(const Limbs9 &a, const Limbs9 &b) { Limbs9 r{}; for (int i = 0; i < 9; i++) r.l[i] = a.l[i] > b.l[i] ? a.l[i] : b.l[i]; return r; }
struct LbNone { static constexpr Limbs9 B = lb_uniform(0); };                 // no such operand
struct LbNorm { static constexpr Limbs9 B = lb_uniform(M29); };               // normalised: out of a column chain or normw, value < 2^261
struct LbAny { static constexpr Limbs9 B = lb_uniform(0xffffffffu); };        // an addend as it stands (a padded difference, not normalised)
struct LbMulwA { static constexpr Limbs9 B = lb_uniform(MULW_A_LIMB_MAX); };  // the left operand of a masked product: a sum or a padded difference
struct LbBelow30 { static constexpr Limbs9 B = lb_uniform((1u << 30) - 1); }; // a sum of two normalised values
constexpr unsigned LZ_ALL = 0xffu;
constexpr bool lazy_digit(unsigned lz, int k) { return k < 8 && ((lz >> k) & 1u); }
struct ColBound { uint64_t worst; bool fits; };                // the largest column (wrapped if it does not fit); all columns below 2^64
// columns of a*b + c*d + e*f + m~*p (+ addend in the high columns), m~ with the digits of lz unmasked.  A squaring is a = b = the operand's
// bounds: the doubled cross products and the square of a column sum to the same worst case.
// fold: the set of folded digits and fc the limbs of 2^-29 mod p they are multiplied by (digit i: fc[j] in column i + 1 + j, nothing in column i)
constexpr bool fold_digit(unsigned fold, int k) { return k >= 0 && k < 32 && ((fold >> k) & 1u); }
constexpr ColBound lazy_col_bound(const Limbs9 &a, const Limbs9 &b, const Limbs9 &c, const Limbs9 &d, const Limbs9 &addend, const uint32_t (&p)[9], unsigned lz,
                                  const Limbs9 &e = LbNone::B, const Limbs9 &f = LbNone::B, unsigned fold = 0, const Limbs9 &fc = LbNone::B) {
    uint64_t carry = 0, worst = 0;
    bool fits = true;
    for (int k = 0; k < 17; k++) {
        uint64_t s = carry;
        for (int i = (k < 9 ? 0 : k - 8); i <= (k < 9 ? k : 8); i++) {
            fits &= !__builtin_add_overflow(s, (uint64_t)a.l[k - i] * b.l[i], &s);
            fits &= !__builtin_add_overflow(s, (uint64_t)c.l[k - i] * d.l[i], &s);
            fits &= !__builtin_add_overflow(s, (uint64_t)e.l[k - i] * f.l[i], &s);
            if (!fold_digit(fold, i)) fits &= !__builtin_add_overflow(s, (uint64_t)(lazy_digit(lz, i) ? 0xffffffffu : M29) * p[k - i], &s);
        }
        for (int i = 0; i < 9; i++)
            if (fold_digit(fold, i) && k - i - 1 >= 0 && k - i - 1 <= 8) fits &= !__builtin_add_overflow(s, (uint64_t)(lazy_digit(lz, i) ? 0xffffffffu : M29) * fc.l[k - i - 1], &s);
        if (k >= 9) fits &= !__builtin_add_overflow(s, (uint64_t)addend.l[k - 9], &s);
        if (s > worst) worst = s;
        carry = s >> 29;
    }
    return ColBound{worst, fits};
}
#define PLK_LZ_DIGIT(LZ, k, acc) (lazy_digit((LZ), (k)) ? (uint32_t)(acc) * WP::INV29 : ((uint32_t)(acc) * WP::INV29) & M29)
// a fold set of a reduction of D digits is sound: a prefix 0..f-1, f <= D - 2 (each folded digit divided by 2^58 or more), and what the set can add to
// the result, below 2^32 (C_8 + 1) 2^232 / 2^58 (1 + 2^-28), at most 2^-24 p, p >= p_8 2^232:  (C_8 + 1) (2^28 + 1) <= p_8 2^30
constexpr bool fold_value_ok(unsigned fold, int digits, const uint32_t (&c)[9], const uint32_t (&p)[9]) {
    if (fold == 0) return true;
    if ((fold & (fold + 1)) != 0) return false;
    int f = 0;
    while ((fold >> f) & 1u) f++;
    return f <= digits - 2 && ((uint64_t)c[8] + 1) * ((1ull << 28) + 1) <= ((uint64_t)p[8] << 30);
}
// c is 2^-29 mod p as nine limbs below 2^29: c 2^29 - 1 = q p with q < 2^58, whose two digits follow from the low limbs (q_k = n_k / p mod 2^29, as
// in an exact division from the low end); what is left after q p is taken away must be zero
constexpr bool foldc_ok(const uint32_t (&c)[9], const uint32_t (&p)[9], uint32_t pinv0) {
    int64_t n[12] = {};
    for (int i = 0; i < 9; i++) { if (c[i] > M29) return false; n[i + 1] = c[i]; }
    n[0] = -1;
    for (int i = 0; i < 11; i++) { int64_t cy = n[i] >> 29; n[i] &= (int64_t)M29; n[i + 1] += cy; }   // normalise c 2^29 - 1 (non-negative: c > 0)
    for (int k = 0; k < 2; k++) {
        const int64_t q = (int64_t)(((uint64_t)n[k] * pinv0) & M29);
        int64_t cy = 0;
        for (int j = k; j < 12; j++) {
            const int64_t s = n[j] - (j - k < 9 ? q * (int64_t)p[j - k] : 0) + cy;
            n[j] = s & (int64_t)M29;
            cy = s >> 29;
            if (j == 11) n[j] = s;
        }
    }
    for (int i = 0; i < 12; i++) if (n[i] != 0) return false;
    return true;
}
static_assert(foldc_ok(FqW::FOLDC, FqW::P29, FqW::PINV0), "FqW::FOLDC is not 2^-29 mod p below 2^261");
static_assert(foldc_ok(FrW::FOLDC, FrW::P29, FrW::PINV0), "FrW::FOLDC is not 2^-29 mod p below 2^261");
#define PLK_FOLD_MSG "a fold set is a prefix of the digits short of the last two, and adds at most 2^-24 p to the result"

// the second chain of a scan that has only one: every step is nothing
struct NoChain {
    static constexpr bool FITS = true;
    static constexpr bool FOLD_OK = true;
    static constexpr unsigned FOLD = 0;
    uint32_t m[9];
    uint64_t acc;
    PLK_HD void mad(uint64_t, uint32_t) {}
    PLK_HD void mp(int, int) {}
    PLK_HD void digit(int) {}
    PLK_HD void mp0(int) {}
    PLK_HD void addend(int) {}
    PLK_HD void limb(int) {}
    PLK_HD void shift(int) {}
    PLK_HD void top() {}
};
// one accumulator chain of the scan: its operand half, its result, its addend if LAD is not LbNone (limb j joins the accumulator at
// column 9 + j, after the column's m*p terms and before output limb j is cut off), its digits and its accumulator
// (FLD: the set of folded digits, "THE FOLD" above; mp(k, i) is digit i's term of column k > i, m_i * p_(k-i) or, folded, m_i * C_(k-i-1))
template <class WP, unsigned LZ, class H, class LAD = LbNone, unsigned FLD = 0>
struct MontChain {
    using Half = H;
    static constexpr unsigned FOLD = FLD;
    static constexpr bool ADD = !std::is_same<LAD, LbNone>::value;
    static constexpr bool FITS = H::bound(LAD::B, LZ, FLD).fits;
    static constexpr bool FOLD_OK = fold_value_ok(FLD, 9, WP::FOLDC, WP::P29);
    H h;
    const W9<WP> *A = nullptr;
    W9<WP> *r = nullptr;
    uint32_t m[9];
    uint64_t acc = 0;
    PLK_HD void mad(uint64_t a, uint32_t b) { acc += a * b; PLK_CHAIN(acc); }
    PLK_HD void mp(int k, int i) {
        if (fold_digit(FLD, i)) mad(m[i], WP::FOLDC[k - i - 1]);
        else if (k - i <= 8) mad(m[i], WP::P29[k - i]);
    }
    PLK_HD void digit(int k) {
        if (fold_digit(FLD, k)) m[k] = lazy_digit(LZ, k) ? (uint32_t)acc : (uint32_t)acc & M29;
        else m[k] = PLK_LZ_DIGIT(LZ, k, acc);
    }
    PLK_HD void mp0(int k) { if (!fold_digit(FLD, k)) acc += (uint64_t)m[k] * WP::P29[0]; }
    PLK_HD void limb(int k) { r->l[k - 9] = (uint32_t)acc & M29; }
    PLK_HD void shift(int k) {
        if (fold_digit(FLD, k) && lazy_digit(LZ, k)) PLK_FOLD_CARRY(acc)
        else acc >>= 29;
    }
    PLK_HD void addend(int k) { if constexpr (ADD) PLK_ADDEND(acc, A->l[k - 9]); }
    PLK_HD void top() { r->l[8] = (uint32_t)acc; if constexpr (ADD) r->l[8] += A->l[8]; }
};
// The operand halves: what column k receives besides m*p.  The scan walks i = lo .. while more(k, i, hi) and takes term<0..2>(chain, k, i)
// of each chain in turn, then last(chain, k) where has_last<LOW>(k); prepare(chain, j) runs once per limb before the scan.  They hold no loop
// of their own (see mont_scan); bound: the worst columns with every operand at its declared bound.
// T = 1, 2 or 3 products a_t * b_t; x = {a_0, b_0, a_1, b_1, ...} and L their declared bounds in that order.  a_t[k - i] * b_t[i] for
// t = 0 .. T-1, then the next i.
template <class WP, class... L>
struct Products {
    static constexpr int T = sizeof...(L) / 2;
    const W9<WP> *x[2 * T];
    static PLK_HD bool more(int k, int i, int hi) { return i <= hi; }
    template <int J, class C> static PLK_HD void term(C &c, int k, int i) {
        if constexpr (J < T && !std::is_same<C, NoChain>::value) c.mad(c.h.x[2 * J]->l[k - i], c.h.x[2 * J + 1]->l[i]);
    }
    template <class C> static PLK_HD void prepare(C &, int) {}
    template <class C> static PLK_HD void last(C &, int) {}
    template <bool LOW> static PLK_HD bool has_last(int) { return false; }
    static constexpr ColBound bound(const Limbs9 &addend, unsigned lz, unsigned fold = 0) {
        const Limbs9 b[6] = {L::B...};                         // (the pairs that are not there: zeros)
        return lazy_col_bound(b[0], b[1], b[2], b[3], addend, WP::P29, lz, b[4], b[5], fold, lb_of(WP::FOLDC));
    }
};
// x^2: the cross products x_i*x_j (i < j) are taken once against the doubled operand, then the square on an even column: 45 + 81
// multiply-adds instead of 162.  LX: the declared bound of x (below 2^31: the doubled limb is a 32-bit value)
template <class WP, class LX>
struct Squaring {
    static_assert(lb_below(LX::B, 1u << 31), "a doubled limb can exceed 32 bits");
    const W9<WP> &x;
    uint32_t d[9];
    static PLK_HD bool more(int k, int i, int) { return 2 * i < k; }
    template <int J, class C> static PLK_HD void term(C &c, int k, int i) {
        if constexpr (J == 0 && !std::is_same<C, NoChain>::value) c.mad(c.h.d[k - i], c.h.x.l[i]);
    }
    template <class C> static PLK_HD void prepare(C &c, int j) { if constexpr (!std::is_same<C, NoChain>::value) c.h.d[j] = c.h.x.l[j] << 1; }
    template <class C> static PLK_HD void last(C &c, int k) { if constexpr (!std::is_same<C, NoChain>::value) c.mad(c.h.x.l[k / 2], c.h.x.l[k / 2]); }
    template <bool LOW> static PLK_HD bool has_last(int k) { return k % 2 == 0; }
    static constexpr ColBound bound(const Limbs9 &addend, unsigned lz, unsigned fold = 0) {
        return lazy_col_bound(LX::B, LX::B, LbNone::B, LbNone::B, addend, WP::P29, lz, LbNone::B, LbNone::B, fold, lb_of(WP::FOLDC));
    }
};
// x * 2^5 (canonical_w): x_k << 5 in column k — nine shifts, no multiply-add.  As a product it is x times the limbs (32, 0, ..., 0).
template <class WP>
struct Shift5 {
    const W9<WP> &x;
    static PLK_HD bool more(int, int, int) { return false; }
    template <int J, class C> static PLK_HD void term(C &, int, int) {}
    template <class C> static PLK_HD void prepare(C &, int) {}
    template <class C> static PLK_HD void last(C &c, int k) { if constexpr (!std::is_same<C, NoChain>::value) c.acc += (uint64_t)c.h.x.l[k] << 5; }
    template <bool LOW> static PLK_HD bool has_last(int) { return LOW; }
    static constexpr ColBound bound(const Limbs9 &addend, unsigned lz, unsigned fold = 0) {
        return lazy_col_bound(LbNorm::B, Limbs9{{32}}, LbNone::B, LbNone::B, addend, WP::P29, lz, LbNone::B, LbNone::B, fold, lb_of(WP::FOLDC));
    }
};
// THE scan.  Order is the contract (it is what the schedule and the register count of every hot kernel hang on): inside a column every
// step goes chain 0, chain 1 — the operand half's terms one by one, the m*p terms one by one, then both digits, both m*p_0, both
// shifts; in a high column both addends, both limbs, both shifts.  The chains' state (digits, accumulator) is LOCAL to this function, and
// chain 0's result is its return value: with the state or the result of a single chain handed in from a caller the compiler schedules
// every kernel differently (profiles/field29_engine_isa.txt).  The loops must unroll: the limb arrays are registers only then.
template <class WP, class C0, class C1 = NoChain>
PLK_HD auto mont_scan(const C0 &s0, const C1 &s1 = C1{}, W9<WP> *r0 = nullptr, W9<WP> *r1 = nullptr) {
    static_assert(C0::FITS, "a column of chain 0 can exceed 64 bits");
    static_assert(C1::FITS, "a column of chain 1 can exceed 64 bits");
    static_assert(C0::FOLD_OK && C1::FOLD_OK, PLK_FOLD_MSG);
    using H = typename C0::Half;
    constexpr bool ONE = std::is_same<C1, NoChain>::value;     // one chain: the result is returned; two: written to r0, r1
    W9<WP> r;
    C0 c0 = s0;
    C1 c1 = s1;
    if constexpr (ONE) c0.r = &r;
    else { c0.r = r0; c1.r = r1; }
#pragma unroll
    for (int j = 0; j < 9; j++) { H::prepare(c0, j); H::prepare(c1, j); }
#pragma unroll
    for (int k = 0; k < 9; k++) {
#pragma unroll
        for (int i = 0; H::more(k, i, k); i++) { H::template term<0>(c0, k, i); H::template term<0>(c1, k, i); H::template term<1>(c0, k, i); H::template term<1>(c1, k, i); H::template term<2>(c0, k, i); H::template term<2>(c1, k, i); }
        if (H::template has_last<true>(k)) { H::last(c0, k); H::last(c1, k); }
#pragma unroll
        for (int i = 0; i < k; i++) { c0.mp(k, i); c1.mp(k, i); }
        c0.digit(k); c1.digit(k);
        c0.mp0(k); c1.mp0(k);
        c0.shift(k); c1.shift(k);
    }
#pragma unroll
    for (int k = 9; k < 17; k++) {
#pragma unroll
        for (int i = k - 8; H::more(k, i, 8); i++) { H::template term<0>(c0, k, i); H::template term<0>(c1, k, i); H::template term<1>(c0, k, i); H::template term<1>(c1, k, i); H::template term<2>(c0, k, i); H::template term<2>(c1, k, i); }
        if (H::template has_last<false>(k)) { H::last(c0, k); H::last(c1, k); }
#pragma unroll
        for (int i = k - 9; i <= 8; i++) { c0.mp(k, i); c1.mp(k, i); }   // (i = k - 9: a folded digit's last term; nothing for a Montgomery digit)
        c0.addend(k); c1.addend(k);
        c0.limb(k); c1.limb(k);
        c0.shift(k); c1.shift(k);
    }
    c0.top(); c1.top();
    if constexpr (ONE) return r;
}

// ---- the forms with lazy digits.  LA, LB, ...: the declared limb bounds of the operands, in the order of the arguments.  FD: the fold set of
// the form's chains (0: none folded).
// mulw2: two independent products in lockstep
template <class WP, unsigned LZ0, unsigned LZ1, class LA0, class LB0, class LA1, class LB1, unsigned FD = 0>
PLK_HD void mulw2_lz(const W9<WP> &a0, const W9<WP> &b0, const W9<WP> &a1, const W9<WP> &b1, W9<WP> &r0, W9<WP> &r1) {
    mont_scan<WP>(MontChain<WP, LZ0, Products<WP, LA0, LB0>, LbNone, FD>{{{&a0, &b0}}}, MontChain<WP, LZ1, Products<WP, LA1, LB1>, LbNone, FD>{{{&a1, &b1}}}, &r0, &r1);
}
// sqrw2: two independent squarings in lockstep
template <class WP, unsigned LZ0, unsigned LZ1, class LX0, class LX1, unsigned FD = 0>
PLK_HD void sqrw2_lz(const W9<WP> &x0, const W9<WP> &x1, W9<WP> &r0, W9<WP> &r1) {
    mont_scan<WP>(MontChain<WP, LZ0, Squaring<WP, LX0>, LbNone, FD>{{x0}}, MontChain<WP, LZ1, Squaring<WP, LX1>, LbNone, FD>{{x1}}, &r0, &r1);
}
// mulw2_add: the lockstep pair with a 9-limb ADDEND folded into each chain (the mixed addition of msm_accumulate):
//     r_q = a_q * b_q * 2^-261 + A_q,  normalised,   q = 0, 1
// A_q is any 9-limb value (limbs up to 2^32 - 1: a padded difference "PADk - x" as it stands, not normalised).  The column chain that
// normalises the product normalises the sum as well: the result is bit for bit normw(addw(mulw(a, b), A)) — same integer, same (unique)
// normalised form — without the 9 additions and the 25 instructions of normw, for 8 multiply-adds by one (the top limb is a 32-bit add).
// The value must stay below 2^261 and the top limb below 2^32: callers add less than 16p to a product below 1.1p.
template <class WP, unsigned LZ0, unsigned LZ1, class LA0, class LB0, class LAD0, class LA1, class LB1, class LAD1, unsigned FD = 0>
PLK_HD void mulw2_add_lz(const W9<WP> &a0, const W9<WP> &b0, const W9<WP> &A0, const W9<WP> &a1, const W9<WP> &b1, const W9<WP> &A1, W9<WP> &r0, W9<WP> &r1) {
    mont_scan<WP>(MontChain<WP, LZ0, Products<WP, LA0, LB0>, LAD0, FD>{{{&a0, &b0}}, &A0}, MontChain<WP, LZ1, Products<WP, LA1, LB1>, LAD1, FD>{{{&a1, &b1}}, &A1}, &r0, &r1);
}
// mul2addw: a*b + c*d with ONE Montgomery reduction (243 mads instead of 324).  Used as a*b - c*e by passing d = k*p - e.
template <class WP, unsigned LZ, class LA, class LB, class LC, class LD, unsigned FD = 0>
PLK_HD W9<WP> mul2addw_lz(const W9<WP> &a, const W9<WP> &b, const W9<WP> &c, const W9<WP> &d) {
    return mont_scan<WP>(MontChain<WP, LZ, Products<WP, LA, LB, LC, LD>, LbNone, FD>{{{&a, &b, &c, &d}}});
}

// ---- the masked forms: the same with no digit unmasked and the bounds of their contracts.
// mulw(a, b): b normalised; a may be an un-normalised sum or padded difference with limbs up to MULW_A_LIMB_MAX — the sums the kernels
// feed in: x + y (< 2^30), x + PAD2 - y (< 2^29 + 2.66e9 = 3.19e9).
template <class WP>
PLK_HD W9<WP> mulw(const W9<WP> &a, const W9<WP> &b) { return mont_scan<WP>(MontChain<WP, 0, Products<WP, LbMulwA, LbNorm>>{{{&a, &b}}}); }
template <class WP>
PLK_HD void mulw2(const W9<WP> &a0, const W9<WP> &b0, const W9<WP> &a1, const W9<WP> &b1, W9<WP> &r0, W9<WP> &r1) {
    mulw2_lz<WP, 0, 0, LbMulwA, LbNorm, LbMulwA, LbNorm>(a0, b0, a1, b1, r0, r1);
}
template <class WP>
PLK_HD void mulw2_add(const W9<WP> &a0, const W9<WP> &b0, const W9<WP> &A0, const W9<WP> &a1, const W9<WP> &b1, const W9<WP> &A1, W9<WP> &r0, W9<WP> &r1) {
    mulw2_add_lz<WP, 0, 0, LbMulwA, LbNorm, LbAny, LbMulwA, LbNorm, LbAny>(a0, b0, A0, a1, b1, A1, r0, r1);
}
// normalised input
template <class WP>
PLK_HD W9<WP> sqrw(const W9<WP> &a) { return mont_scan<WP>(MontChain<WP, 0, Squaring<WP, LbNorm>>{{a}}); }
template <class WP>
PLK_HD void sqrw2(const W9<WP> &x0, const W9<WP> &x1, W9<WP> &r0, W9<WP> &r1) { sqrw2_lz<WP, 0, 0, LbNorm, LbNorm>(x0, x1, r0, r1); }
// limbs: a, c < 2^30; b, d < 2^29
template <class WP>
PLK_HD W9<WP> mul2addw(const W9<WP> &a, const W9<WP> &b, const W9<WP> &c, const W9<WP> &d) {
    return mul2addw_lz<WP, 0, LbBelow30, LbNorm, LbBelow30, LbNorm>(a, b, c, d);
}
// a0*b0 + a1*b1 + a2*b2 with one reduction (3*81 + 81 mads instead of 3*162).  Normalised inputs.
template <class WP>
PLK_HD W9<WP> mulsum3w(const W9<WP> &a0, const W9<WP> &b0, const W9<WP> &a1, const W9<WP> &b1, const W9<WP> &a2, const W9<WP> &b2) {
    return mont_scan<WP>(MontChain<WP, 0, Products<WP, LbNorm, LbNorm, LbNorm, LbNorm, LbNorm, LbNorm>>{{{&a0, &b0, &a1, &b1, &a2, &b2}}});
}

// ---- product by a CONSTANT that is held as three shifted copies ("tw3"): 108 multiply-adds instead of 162.
// For a constant w keep  W_q = w * 2^(87 (q+1)) mod p  (q = 0, 1, 2; canonical, 9 limbs each).  Split the variable operand into
// three chunks of three limbs, x = X_0 + X_1 2^87 + X_2 2^174: then  X_0 W_0 + X_1 W_1 + X_2 W_2 = x * w * 2^87 (mod p)  and all
// three partial products start at column 0, so only THREE Montgomery steps (one per limb of 2^87) are needed to divide the 2^87
// out again:
//     mul_tw3(x, W) = (X_0 W_0 + X_1 W_1 + X_2 W_2 + m p) / 2^87  =  x * w  (mod p),      81 + 27 multiply-adds, 12 columns.
// The constant costs 27 words instead of 9 — this is for constants that are read from a table many times (the NTT's stage
// twiddles); no domain change: the result is in whatever domain x is in, w is the PLAIN value of the constant.
// Bounds: a column holds at most 9 products x_j * W (x_j <= A, W < 2^29), 3 products m * p and a carry:
// 9 A (2^29 - 1) + 3 (2^29 - 1)^2 + 2^35 < 2^64 for A <= 3.6e9 (MULTW3_X_LIMB_MAX).  The result depends on the chunk values, not on
// the value of x: r < (X_0 + X_1 + X_2 + 2^87) p / 2^87, i.e. r < 4p for NORMALISED x (limbs < 2^29, so X_q < 2^87) — un-normalised
// limbs are allowed but buy a bound of up to 19p (limbs of 3.2e9), so callers normalise first.  Output limbs are normalised.
constexpr uint32_t MULTW3_X_LIMB_MAX = 3600000000u;
template <class WP> struct Tw3 { uint32_t w[3][9]; };
// one body for one product, or two by the SAME constant in lockstep (as mont_scan: the multiply-adds of the chains alternate one by
// one, the state is local, one chain's result is the return value)
template <class WP>
struct Tw3Chain {
    const W9<WP> &x;
    W9<WP> *r = nullptr;
    uint32_t m[3];
    uint64_t acc = 0;
    PLK_HD void mad(uint64_t a, uint32_t b) { acc += a * b; PLK_CHAIN(acc); }
    PLK_HD void xw(int j, uint32_t w) { mad(x.l[j], w); }
    PLK_HD void digit(int k) { m[k] = ((uint32_t)acc * WP::INV29) & M29; }
    PLK_HD void mp0(int k) { acc += (uint64_t)m[k] * WP::P29[0]; }
    PLK_HD void limb(int j) { r->l[j] = (uint32_t)acc & M29; }
    PLK_HD void shift() { acc >>= 29; }
    PLK_HD void top() { r->l[8] = (uint32_t)acc; }
};
struct NoTw3Chain : NoChain { PLK_HD void xw(int, uint32_t) {} PLK_HD void shift() {} };
template <class WP, class C1 = NoTw3Chain>
PLK_HD auto mul_tw3_scan(const Tw3<WP> &t, const Tw3Chain<WP> &s0, const C1 &s1 = C1{}, W9<WP> *r0 = nullptr, W9<WP> *r1 = nullptr) {
    constexpr bool ONE = std::is_same<C1, NoTw3Chain>::value;
    W9<WP> r;
    Tw3Chain<WP> c0 = s0;
    C1 c1 = s1;
    if constexpr (ONE) c0.r = &r;
    else { c0.r = r0; c1.r = r1; }
#pragma unroll
    for (int k = 0; k < 11; k++) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (k - i < 0 || k - i > 8) continue;
#pragma unroll
            for (int q = 0; q < 3; q++) { c0.xw(3 * q + i, t.w[q][k - i]); c1.xw(3 * q + i, t.w[q][k - i]); }
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (i >= k || k - i > 8) continue;
            c0.mad(c0.m[i], WP::P29[k - i]); c1.mad(c1.m[i], WP::P29[k - i]);
        }
        if (k < 3) { c0.digit(k); c1.digit(k); c0.mp0(k); c1.mp0(k); }
        else { c0.limb(k - 3); c1.limb(k - 3); }
        c0.shift(); c1.shift();
    }
    c0.top(); c1.top();
    if constexpr (ONE) return r;
}
template <class WP>
PLK_HD W9<WP> mul_tw3(const W9<WP> &x, const Tw3<WP> &t) { return mul_tw3_scan(t, Tw3Chain<WP>{x}); }
// two of them (the two products of a butterfly stage that share a twiddle)
template <class WP>
PLK_HD void mul_tw3_2(const W9<WP> &x0, const W9<WP> &x1, const Tw3<WP> &t, W9<WP> &r0, W9<WP> &r1) {
    mul_tw3_scan(t, Tw3Chain<WP>{x0}, Tw3Chain<WP>{x1}, &r0, &r1);
}
// the three copies of a constant given in the W domain (w * 2^261, canonical): W_2 is the value itself, W_1 and W_0 are it times
// 2^-87 and 2^-174 — products by the limb-unit vectors 2^174 and 2^87 (mulw divides by 2^261)
template <class WP>
PLK_HD Tw3<WP> make_tw3(const W9<WP> &w_dom_w) {
    W9<WP> e87 = w_zero<WP>(), e174 = w_zero<WP>();
    e87.l[3] = 1; e174.l[6] = 1;
    const W9<WP> w0 = csub_p(mulw(w_dom_w, e87)), w1 = csub_p(mulw(w_dom_w, e174));
    Tw3<WP> t;
    for (int i = 0; i < 9; i++) { t.w[0][i] = w0.l[i]; t.w[1][i] = w1.l[i]; t.w[2][i] = w_dom_w.l[i]; }
    return t;
}

// ---- product by a SHARED FACTOR that is held in two forms ("tw2"): 126 multiply-adds instead of 162.
// For a factor w (W domain, normalised) that is the right operand of several products keep, beside w itself,
//     A = w * 2^-116 mod p = (W_lo + m p) / 2^116 + W_hi        (make_tw2_a: W_lo = limbs 0..3 of w, W_hi = limbs 4..8; FOUR Montgomery steps)
// and split the variable operand after four limbs, z = Z_0 + Z_1 2^116 (Z_0 = limbs 0..3, Z_1 = limbs 4..8).  Z_0 A + Z_1 w = z w 2^-116 (mod p)
// and both partial products start at column 0, so FIVE Montgomery steps divide the remaining 2^145 out:
//     tw2(z; A, w) = (Z_0 A + Z_1 w + m p) / 2^145  =  z * w * 2^-261 (mod p) — what mulw(z, w) is,   36 + 45 + 45 multiply-adds, 13 columns.
// (The 4 + 5 split is what lets the second form be w as it stands; 5 + 4 would need w * 2^29 mod p.)  A costs 36 multiply-adds by p and three
// by one (limbs 1..3 of w join their columns as PLK_ADDEND; limb 0 starts the chain; W_hi is added limb by limb AFTER the chain, so A's limbs
// 0..4 are below 2^30 and not normalised — LbTw2A): a factor used three times (PP in the mixed addition) pays it back twice over.
// Lazy digits as in mont_scan: the top digit (3 for A, 4 for tw2) is always masked, the others may stay unmasked (bit k of LZ for m_k), so
// m~ < 2^(29 D) (1 + 2^-26) for D digits.  Values, for normalised z and w:
//     A < w / 2^116 + p (1 + 2^-26)                                 (W_lo / 2^116 < 1; in the W domain w < 2^261, so A < 1.0001 p)
//     tw2 < z w / 2^261 + A / 2^29 + p (1 + 2^-26)                  (Z_0 < 2^116, Z_1 2^116 <= z): the bound of mulw2_lz + 2^-28 p.
// Columns: at most 4 products z * A, 5 products z * w, 5 products m~ * p and a carry; every instantiation evaluates its exact worst case at the
// declared limb bounds at compile time (tw2_col_bound, tw2a_col_bound — lazy_col_bound's method) and does not compile if a column can reach 2^64.
// A sibling of mont_scan, as mul_tw3_scan is: the column ranges and the number of digits differ, and mont_scan's text is what the schedule of
// every hot kernel hangs on.  Chain order inside a column is mont_scan's (chain 0, chain 1, one step each).
struct LbTw2A { static constexpr Limbs9 B = Limbs9{{(1u << 30) - 1, (1u << 30) - 1, (1u << 30) - 1, (1u << 30) - 1, (1u << 30) - 1, M29, M29, M29, M29}}; };
constexpr unsigned TW2_LZ_ALL = 0xfu;                          // tw2: m_0..m_3 unmasked
constexpr unsigned TW2A_LZ_ALL = 0x7u;                         // make_tw2_a: m_0..m_2 unmasked
constexpr unsigned FOLD9 = 0x7fu, FOLD_TW2 = 0x7u, FOLD_TW2A = 0x3u;   // the largest fold sets: digits 0..6 of nine, 0..2 of tw2's five, 0..1 of make_tw2_a's four
constexpr ColBound tw2_col_bound(const Limbs9 &z, const Limbs9 &a, const Limbs9 &w, const uint32_t (&p)[9], unsigned lz, unsigned fold = 0, const Limbs9 &fc = LbNone::B) {
    uint64_t carry = 0, worst = 0;
    bool fits = true;
    for (int k = 0; k < 13; k++) {
        uint64_t s = carry;
        for (int i = 0; i < 4; i++) if (k - i >= 0 && k - i <= 8) fits &= !__builtin_add_overflow(s, (uint64_t)z.l[i] * a.l[k - i], &s);
        for (int i = 0; i < 5; i++) if (k - i >= 0 && k - i <= 8) fits &= !__builtin_add_overflow(s, (uint64_t)z.l[4 + i] * w.l[k - i], &s);
        for (int i = 0; i < 5; i++) {
            const uint64_t dg = i < 4 && ((lz >> i) & 1u) ? 0xffffffffu : M29;
            if (!fold_digit(fold, i) && k - i >= 0 && k - i <= 8) fits &= !__builtin_add_overflow(s, dg * p[k - i], &s);
            if (fold_digit(fold, i) && k - i - 1 >= 0 && k - i - 1 <= 8) fits &= !__builtin_add_overflow(s, dg * fc.l[k - i - 1], &s);
        }
        if (s > worst) worst = s;
        carry = s >> 29;
    }
    return ColBound{worst, fits};
}
constexpr ColBound tw2a_col_bound(const Limbs9 &w, const uint32_t (&p)[9], unsigned lz, unsigned fold = 0, const Limbs9 &fc = LbNone::B) {
    uint64_t carry = 0, worst = 0;
    bool fits = true;
    for (int k = 0; k < 12; k++) {
        uint64_t s = carry;
        if (k < 4) fits &= !__builtin_add_overflow(s, (uint64_t)w.l[k], &s);
        for (int i = 0; i < 4; i++) {
            const uint64_t dg = i < 3 && ((lz >> i) & 1u) ? 0xffffffffu : M29;
            if (!fold_digit(fold, i) && k - i >= 0 && k - i <= 8) fits &= !__builtin_add_overflow(s, dg * p[k - i], &s);
            if (fold_digit(fold, i) && k - i - 1 >= 0 && k - i - 1 <= 8) fits &= !__builtin_add_overflow(s, dg * fc.l[k - i - 1], &s);
        }
        if (s > worst) worst = s;
        carry = s >> 29;
    }
    return ColBound{worst, fits};
}
// A = w * 2^-116 mod p.  LW: the declared bound of w (its limbs 4..8 below 2^29 for LbTw2A to hold: static_assert).  One chain: every
// multiply-add reads the one before it.
template <class WP, unsigned LZ = TW2A_LZ_ALL, class LW = LbNorm, unsigned FD = 0>
PLK_HD W9<WP> make_tw2_a(const W9<WP> &w) {
    static_assert(tw2a_col_bound(LW::B, WP::P29, LZ, FD, lb_of(WP::FOLDC)).fits, "a column of make_tw2_a can exceed 64 bits");
    static_assert(fold_value_ok(FD, 4, WP::FOLDC, WP::P29), PLK_FOLD_MSG);
    static_assert(lb_below(LW::B, 1u << 29), "make_tw2_a: the high limbs of w are added to normalised limbs and must stay below 2^30");
    W9<WP> r;
    uint32_t m[4];
    uint64_t acc = w.l[0];
#pragma unroll
    for (int k = 0; k < 12; k++) {
        if (k > 0 && k < 4) PLK_ADDEND(acc, w.l[k]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i >= k || k - i > (fold_digit(FD, i) ? 9 : 8)) continue;
            acc += (uint64_t)m[i] * (fold_digit(FD, i) ? WP::FOLDC[k - i - 1] : WP::P29[k - i]); PLK_CHAIN(acc);
        }
        const bool lzk = k < 3 && ((LZ >> k) & 1u);
        if (fold_digit(FD, k)) m[k] = lzk ? (uint32_t)acc : (uint32_t)acc & M29;                  // (fold_value_ok: k < 2)
        else if (k < 4) {
            m[k] = lzk ? (uint32_t)acc * WP::INV29 : ((uint32_t)acc * WP::INV29) & M29;
            acc += (uint64_t)m[k] * WP::P29[0];
        } else r.l[k - 4] = (uint32_t)acc & M29;
        if (fold_digit(FD, k) && lzk) PLK_FOLD_CARRY(acc)
        else acc >>= 29;
    }
    r.l[8] = (uint32_t)acc;
#pragma unroll
    for (int j = 0; j < 5; j++) r.l[j] += w.l[4 + j];
    return r;
}
// one accumulator chain of the tw2 scan: z, the two forms of its factor, the result
template <class WP, unsigned LZ, class LZV, class LA, class LW, unsigned FLD = 0>
struct Tw2Chain {
    static constexpr unsigned FOLD = FLD;
    static constexpr bool FITS = tw2_col_bound(LZV::B, LA::B, LW::B, WP::P29, LZ, FLD, lb_of(WP::FOLDC)).fits;
    static constexpr bool FOLD_OK = fold_value_ok(FLD, 5, WP::FOLDC, WP::P29);
    const W9<WP> &z, &a, &w;
    W9<WP> *r = nullptr;
    uint32_t m[5];
    uint64_t acc = 0;
    PLK_HD void mad(uint64_t x, uint32_t y) { acc += x * y; PLK_CHAIN(acc); }
    PLK_HD void za(int i, int j) { mad(z.l[i], a.l[j]); }
    PLK_HD void zw(int i, int j) { mad(z.l[4 + i], w.l[j]); }
    PLK_HD void mp(int k, int i) {
        if (fold_digit(FLD, i)) mad(m[i], WP::FOLDC[k - i - 1]);
        else if (k - i <= 8) mad(m[i], WP::P29[k - i]);
    }
    static constexpr bool lzd(int k) { return k < 4 && ((LZ >> k) & 1u); }
    PLK_HD void digit(int k) {
        if (fold_digit(FLD, k)) m[k] = lzd(k) ? (uint32_t)acc : (uint32_t)acc & M29;
        else m[k] = lzd(k) ? (uint32_t)acc * WP::INV29 : ((uint32_t)acc * WP::INV29) & M29;
    }
    PLK_HD void mp0(int k) { if (!fold_digit(FLD, k)) acc += (uint64_t)m[k] * WP::P29[0]; }
    PLK_HD void limb(int j) { r->l[j] = (uint32_t)acc & M29; }
    PLK_HD void shift(int k) {
        if (fold_digit(FLD, k) && lzd(k)) PLK_FOLD_CARRY(acc)
        else acc >>= 29;
    }
    PLK_HD void top() { r->l[8] = (uint32_t)acc; }
};
struct NoTw2Chain : NoChain { PLK_HD void za(int, int) {} PLK_HD void zw(int, int) {} };
template <class WP, class C0, class C1 = NoTw2Chain>
PLK_HD auto mul_tw2_scan(const C0 &s0, const C1 &s1 = C1{}, W9<WP> *r0 = nullptr, W9<WP> *r1 = nullptr) {
    static_assert(C0::FITS, "a column of chain 0 can exceed 64 bits");
    static_assert(C1::FITS, "a column of chain 1 can exceed 64 bits");
    static_assert(C0::FOLD_OK && C1::FOLD_OK, PLK_FOLD_MSG);
    constexpr bool ONE = std::is_same<C1, NoTw2Chain>::value;
    W9<WP> r;
    C0 c0 = s0;
    C1 c1 = s1;
    if constexpr (ONE) c0.r = &r;
    else { c0.r = r0; c1.r = r1; }
#pragma unroll
    for (int k = 0; k < 13; k++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (k - i < 0 || k - i > 8) continue;
            c0.za(i, k - i); c1.za(i, k - i);
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {
            if (k - i < 0 || k - i > 8) continue;
            c0.zw(i, k - i); c1.zw(i, k - i);
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {
            if (i >= k || k - i > 9) continue;
            c0.mp(k, i); c1.mp(k, i);
        }
        if (k < 5) { c0.digit(k); c1.digit(k); c0.mp0(k); c1.mp0(k); }
        else { c0.limb(k - 5); c1.limb(k - 5); }
        c0.shift(k); c1.shift(k);
    }
    c0.top(); c1.top();
    if constexpr (ONE) return r;
}
// z * w * 2^-261 (mod p) with a = make_tw2_a(w); LZV, LA, LW: the declared limb bounds of z, a, w
template <class WP, unsigned LZ = 0, class LZV = LbNorm, class LA = LbTw2A, class LW = LbNorm, unsigned FD = 0>
PLK_HD W9<WP> mul_tw2(const W9<WP> &z, const W9<WP> &a, const W9<WP> &w) { return mul_tw2_scan<WP>(Tw2Chain<WP, LZ, LZV, LA, LW, FD>{z, a, w}); }
// two in lockstep, each by a factor of its own (the same one twice where two products share it)
template <class WP, unsigned LZ0, unsigned LZ1, class LZV0 = LbNorm, class LZV1 = LbNorm, class LA = LbTw2A, class LW = LbNorm, unsigned FD = 0>
PLK_HD void mul_tw2_2(const W9<WP> &z0, const W9<WP> &a0, const W9<WP> &w0, const W9<WP> &z1, const W9<WP> &a1, const W9<WP> &w1, W9<WP> &r0, W9<WP> &r1) {
    mul_tw2_scan<WP>(Tw2Chain<WP, LZ0, LZV0, LA, LW, FD>{z0, a0, w0}, Tw2Chain<WP, LZ1, LZV1, LA, LW, FD>{z1, a1, w1}, &r0, &r1);
}
// a tw2 product (chain 0, 13 columns) in lockstep with a plain Montgomery product a * b (chain 1, a MontChain over ONE product, 17 columns): for
// a pair of which only one factor has its second form.  Column k of both is issued together, the multiply-adds alternating one by one while
// both have some left (term t of column k of each chain, in the order of their own scans); columns 13..16 are chain 1's alone.
// (term t of a column as a compile-time code, kind * 16 + i, or -1 past the column's last: left to the optimiser the scan stays a rolled loop)
// (a folded digit i has its last term in column i + 9, a Montgomery digit in column i + 8)
constexpr int tw2_term_code(int k, int t, unsigned fold = 0) {
    int n = 0;
    for (int i = 0; i < 4; i++) if (k - i >= 0 && k - i <= 8) { if (n == t) return i; n++; }
    for (int i = 0; i < 5; i++) if (k - i >= 0 && k - i <= 8) { if (n == t) return 16 + i; n++; }
    for (int i = 0; i < 5; i++) if (i < k && k - i <= (fold_digit(fold, i) ? 9 : 8)) { if (n == t) return 32 + i; n++; }
    return -1;
}
constexpr int mont_term_code(int k, int t, unsigned fold = 0) {
    const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8;
    int n = 0;
    for (int i = lo; i <= hi; i++) { if (n == t) return i; n++; }
    for (int i = (k < 9 ? 0 : k - 9); i <= hi && i < k; i++) if (k - i <= (fold_digit(fold, i) ? 9 : 8)) { if (n == t) return 16 + i; n++; }
    return -1;
}
// (static_for for code that the host checks compile too)
template <int... J, class F> PLK_HD void static_for_hd_impl(std::integer_sequence<int, J...>, F &&f) { (f(std::integral_constant<int, J>{}), ...); }
template <int N, class F> PLK_HD void static_for_hd(F &&f) { static_for_hd_impl(std::make_integer_sequence<int, N>{}, static_cast<F &&>(f)); }
template <class WP, class CT, class CM>
PLK_HD void mul_tw2_mulw_scan(const CT &s0, const CM &s1, W9<WP> *r0, W9<WP> *r1) {
    static_assert(CT::FITS, "a column of chain 0 can exceed 64 bits");
    static_assert(CM::FITS, "a column of chain 1 can exceed 64 bits");
    static_assert(CM::Half::T == 1 && !CM::ADD, "chain 1 is one product without an addend");
    static_assert(CT::FOLD_OK && CM::FOLD_OK, PLK_FOLD_MSG);
    CT c0 = s0;
    CM c1 = s1;
    c0.r = r0; c1.r = r1;
    static_for_hd<17>([&](auto K) {
        constexpr int k = decltype(K)::value;
        static_for_hd<18>([&](auto T) {
            constexpr int t = decltype(T)::value;
            constexpr int e0 = k < 13 ? tw2_term_code(k, t, CT::FOLD) : -1, e1 = mont_term_code(k, t, CM::FOLD);
            if constexpr (e0 >= 32) c0.mp(k, e0 - 32);
            else if constexpr (e0 >= 16) c0.zw(e0 - 16, k - (e0 - 16));
            else if constexpr (e0 >= 0) c0.za(e0, k - e0);
            if constexpr (e1 >= 16) c1.mp(k, e1 - 16);
            else if constexpr (e1 >= 0) c1.mad(c1.h.x[0]->l[k - e1], c1.h.x[1]->l[e1]);
        });
        if constexpr (k < 5) c0.digit(k);
        if constexpr (k < 9) c1.digit(k);
        if constexpr (k < 5) c0.mp0(k);
        if constexpr (k < 9) c1.mp0(k);
        if constexpr (k >= 5 && k < 13) c0.limb(k - 5);
        if constexpr (k >= 9) c1.limb(k);
        if constexpr (k < 13) c0.shift(k);
        c1.shift(k);
        if constexpr (k == 12) c0.top();
    });
    c1.top();
}
// r0 = tw2(z; a, w), r1 = x * y * 2^-261, in lockstep
template <class WP, unsigned LZ0, unsigned LZ1, class LZV = LbNorm, class LX = LbNorm, class LY = LbNorm, class LA = LbTw2A, class LW = LbNorm, unsigned FD0 = 0, unsigned FD1 = 0>
PLK_HD void mul_tw2_mulw(const W9<WP> &z, const W9<WP> &a, const W9<WP> &w, const W9<WP> &x, const W9<WP> &y, W9<WP> &r0, W9<WP> &r1) {
    mul_tw2_mulw_scan<WP>(Tw2Chain<WP, LZ0, LZV, LA, LW, FD0>{z, a, w}, MontChain<WP, LZ1, Products<WP, LX, LY>, LbNone, FD1>{{{&x, &y}}}, &r0, &r1);
}

// ---- OPERAND-SCANNING forms of the same three products (identical results, bit for bit): ten independent 64-bit
// column accumulators per row instead of one chain.  They issue 16 more instructions per product (the carries join their
// columns through v_lshl_add_u64), but a wave that has its SIMD to itself — the bucket-reduction kernels of the MSM are
// chains of dependent full additions run by one or two waves per SIMD — is bound by the dependent-issue latency of a single
// chain (on gfx950 a v_mad_u64_u32 feeding the next one costs a wait state), not by the instruction count: measured, the
// reduction kernels are 15-20 % faster on these forms (msm_task_reduce 0.25 -> 0.21 ms, msm_window_sums 0.13 -> 0.11 at
// 2^20 terms), while every throughput-bound kernel (NTT passes, point-wise kernels, the accumulation) is as fast or faster
// on the product-scanning forms above.
// They share nothing with mont_scan on purpose: the host checks hold the two formulations against each other.  (Each is written out in
// full: with the reduction row or the normalising tail behind a shared function the g1ntt_stage kernels, g1_add_call and msm_naive come out
// with other instruction and register counts or another schedule.)
template <class WP>
PLK_HD W9<WP> mulw_os(const W9<WP> &a, const W9<WP> &b) {
    uint64_t t[10];
#pragma unroll
    for (int j = 0; j < 10; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] += (uint64_t)a.l[j] * b.l[i];
        const uint32_t m = ((uint32_t)t[0] * WP::INV29) & M29;
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] += (uint64_t)m * WP::P29[j];
        const uint64_t c = t[0] >> 29;                               // t[0] is now a multiple of 2^29
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] = t[j + 1];
        t[0] += c;
        t[9] = 0;
    }
    W9<WP> r;
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { uint64_t s = t[j] + c; r.l[j] = (uint32_t)s & M29; c = s >> 29; }
    r.l[8] = (uint32_t)(t[8] + c);
    return r;
}
// a^2: the cross products a_i*a_j (i < j) are taken once against the doubled operand, 45 + 81 mads instead
// of 162.  Row i adds a_i^2 to column 2i and 2*a_j*a_i (j > i) to column i+j; every product that belongs to
// global column g is in place before step g reduces it (the smaller index is <= g/2).
template <class WP>
PLK_HD W9<WP> sqrw_os(const W9<WP> &a) {
    uint64_t t[10];
    uint32_t a2[9];
#pragma unroll
    for (int j = 0; j < 10; j++) t[j] = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) a2[j] = a.l[j] << 1;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        t[i] += (uint64_t)a.l[i] * a.l[i];                           // global column 2i = local column i
#pragma unroll
        for (int j = i + 1; j < 9; j++) t[j] += (uint64_t)a2[j] * a.l[i];   // global column i+j = local column j
        const uint32_t m = ((uint32_t)t[0] * WP::INV29) & M29;
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] += (uint64_t)m * WP::P29[j];
        const uint64_t c = t[0] >> 29;
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] = t[j + 1];
        t[0] += c;
        t[9] = 0;
    }
    W9<WP> r;
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { uint64_t s = t[j] + c; r.l[j] = (uint32_t)s & M29; c = s >> 29; }
    r.l[8] = (uint32_t)(t[8] + c);
    return r;
}

// a*b + c*d with ONE Montgomery reduction (243 mads instead of 324).  Used as a*b - c*e by passing
// d = k*p - e.  Limbs: a, c < 2^30; b, d < 2^29.  Columns hold at most 9 * (2*2^59 + 2^58) < 2^63.4.
template <class WP>
PLK_HD W9<WP> mul2addw_os(const W9<WP> &a, const W9<WP> &b, const W9<WP> &c, const W9<WP> &d) {
    uint64_t t[10];
#pragma unroll
    for (int j = 0; j < 10; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] += (uint64_t)a.l[j] * b.l[i];
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] += (uint64_t)c.l[j] * d.l[i];
        const uint32_t m = ((uint32_t)t[0] * WP::INV29) & M29;
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] += (uint64_t)m * WP::P29[j];
        const uint64_t cy = t[0] >> 29;
#pragma unroll
        for (int j = 0; j < 9; j++) t[j] = t[j + 1];
        t[0] += cy;
        t[9] = 0;
    }
    W9<WP> r;
    uint64_t cy = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { uint64_t s = t[j] + cy; r.l[j] = (uint32_t)s & M29; cy = s >> 29; }
    r.l[8] = (uint32_t)(t[8] + cy);
    return r;
}

// exact conditional subtraction: normalised a < 2p  ->  a mod p in [0, p)
template <class WP>
PLK_HD W9<WP> csub_p(const W9<WP> &a) {
    int32_t d[9];
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { int32_t s = (int32_t)a.l[i] - (int32_t)WP::P29[i] + c; d[i] = s & (int32_t)M29; c = s >> 29; }
    d[8] = (int32_t)a.l[8] - (int32_t)WP::P29[8] + c;
    const bool neg = d[8] < 0;
    W9<WP> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = neg ? a.l[i] : (uint32_t)d[i];
    return r;
}

// full reduction of any normalised value < 2^261 to the canonical residue: one product by 2^261 (the
// Montgomery "one" of this layer) brings it below ~1.01 p, then one exact subtraction
template <class WP>
PLK_HD W9<WP> reduce_full(const W9<WP> &a) { return csub_p(mulw(a, w_one<WP>())); }

// canonical residue of a normalised a < 64p without a product: q = floor(top limb / (top limb of p + 1)) is
// floor(a/p) or one less (the error term is below 1e-5), so a - q*p < 2p and one conditional subtraction ends it.
// ~100 cheap instructions against ~300 for the product by one.
template <class WP>
PLK_HD W9<WP> reduce_small(const W9<WP> &a) {
    const uint32_t q = a.l[8] / (WP::P29[8] + 1u);               // constant divisor: a multiply-high and a shift
    W9<WP> r;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int64_t s = (int64_t)a.l[i] - (int64_t)q * (int64_t)WP::P29[i] + c;
        r.l[i] = (uint32_t)s & M29;
        c = s >> 29;
    }
    r.l[8] = (uint32_t)((int64_t)a.l[8] - (int64_t)q * (int64_t)WP::P29[8] + c);
    return csub_p(r);
}

// a == 0 (mod p) for normalised a < 16p.  a = k*p forces l[0] * p^-1 = k (mod 2^29) with k < 16, which a
// random value passes with probability 2^-25; only then is the value reduced and compared.
template <class WP>
PLK_HD bool is_zero_mod_p(const W9<WP> &a) {
    uint32_t k = (a.l[0] * WP::PINV0) & M29;
    if (k >= 16) return false;
    return w_all_zero(reduce_full(a));
}

// the cheap half of the test above (no false negatives)
template <class WP>
PLK_HD bool maybe_zero_mod_p(const W9<WP> &a) { return ((a.l[0] * WP::PINV0) & M29) < 16; }

// domain changes at the boundary of the W layer (s = packed external form, R = 2^256)
template <class WP> PLK_HD W9<WP> w_from_s(const W9<WP> &raw) { return mulw(raw, w_from_s_const<WP>()); }      // x*2^256 -> x*2^261 (< 1.1p)
template <class WP> PLK_HD W9<WP> s_from_w(const W9<WP> &a) { return csub_p(mulw(a, s_from_w_const<WP>())); }   // x*2^261 -> x*2^256 canonical

// Leaving the EXTERNAL Montgomery form (x * 2^256, any 256-bit value) on this layer: the canonical residue x mod p as nine normalised limbs,
// the same integer as to_canonical() of field_dev.h gives in eight words.  One product-scanning Montgomery pass by the constant 2^5 (the
// layer divides by 2^261): the a*b half is a_k * 2^5 in column k — nine shifts, no multiply-add — and the reduction half the usual 45 + 36.
// The columns fit with room to spare (asserted at mont_scan, like every form's).  The value before the
// subtraction is (32 a + m p) / 2^261 < 1 + p for a < 2^256 and m < 2^261, i.e. at most p, and the CIOS pass of to_canonical() is
// (a + m' p) / 2^256 <= p as well: both end with one conditional subtraction, both are = a * 2^-256 (mod p) and in [0, p), hence equal.
// 81 multiply-adds against the 64 of mul(a, 1), but none of its carry chains (tests/host/field29_pairs_check.hip compares the two).
template <class WP, class PR>
PLK_HD W9<WP> canonical_w(const Fp<PR> &s) {
    const W9<WP> a = unpack<WP>(s);
    return csub_p(mont_scan<WP>(MontChain<WP, 0, Shift5<WP>>{{a}}));
}
PLK_HD W9<FrW> fr_canonical_w(const Fr &k) { return canonical_w<FrW>(k); }

using FrW9 = W9<FrW>;
using FqW9 = W9<FqW>;

}  // namespace plk
