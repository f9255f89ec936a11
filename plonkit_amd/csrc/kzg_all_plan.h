// All openings on the domain in one pass (kzg_all.hip, Feist-Khovratovich): where everything goes, as pure functions of integers.
// No HIP include: the kernels and a stand-alone host program (tests/host/kzg_all_plan_check.cpp) run the same functions.
// NO COUNTERPART IN THE REFERENCE: bellman's kate_commitment opens at one point per call.
//
// f has N = 2^log_n coefficients, the key is s_j = tau^j G.  The quotient commitments
//     h_k = sum_{j = 0}^{N-2-k} f_{k+1+j} s_j   (k <= N - 2),   h_{N-1} = 0
// give every opening at once, pi_i = sum_k h_k omega^(i k) = DFT_N(h)_i, and h is one cyclic correlation of length 2N:
//     c (Fr, 2N)   c_m = f_{m+1} for m <= N - 2, zero elsewhere
//     t (G1, 2N)   t_0 = s_0, t_{2N-j} = s_j for 1 <= j <= N - 2, the identity elsewhere
//     h = the FIRST N entries of iDFT_2N(DFT_2N(c) o DFT_2N(t)), 1 / 2N included; the upper N entries are not zero and are never read.
// Both maps are given from the side of the OUTPUT index (one lane per element of c or t, no scatter).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLK_FK_HD __host__ __device__ inline
#else
#define PLK_FK_HD inline
#endif

namespace plk {

constexpr uint32_t FK_MAX_LOG_N = 25;                              // the 2N-point G1 transforms stay within g1ntt's 2^26
constexpr uint32_t FK_NONE = 0xffffffffu;                          // "zero" in c, "the identity" in t
constexpr size_t FK_FR_BYTES = 32, FK_AFFINE_BYTES = 64, FK_XYZZW_BYTES = 144;
constexpr size_t FK_KEEP_BYTES = (size_t)64 << 20;                 // scratch grown beyond this by a call is released when it returns

// which coefficient of f stands at c[m], m < 2N; FK_NONE: zero
PLK_FK_HD uint32_t fk_c_source(uint32_t log_n, uint32_t m) {
    const uint32_t n = 1u << log_n;
    return m + 2 <= n ? m + 1 : FK_NONE;                           // m <= N - 2
}
// which key point stands at t[m], m < 2N; FK_NONE: the identity
PLK_FK_HD uint32_t fk_t_source(uint32_t log_n, uint32_t m) {
    const uint32_t n = 1u << log_n;
    if (m == 0) return n >= 2 ? 0 : FK_NONE;                       // (N = 1: h is empty, no key point is read)
    const uint32_t j = 2 * n - m;                                  // t_{2N-j} = s_j
    return (j >= 1 && j + 2 <= n) ? j : FK_NONE;                   // 1 <= j <= N - 2
}
// and from the side of the inputs (the statement of the issue; the host check holds the two views against each other)
PLK_FK_HD uint32_t fk_c_index_of_coeff(uint32_t i) { return i ? i - 1 : FK_NONE; }                 // f_0 enters no quotient
PLK_FK_HD uint32_t fk_t_index_of_key(uint32_t log_n, uint32_t j) { return j ? (2u << log_n) - j : 0; }   // for j <= N - 2

PLK_FK_HD bool fk_size_ok(uint32_t log_n) { return log_n <= FK_MAX_LOG_N; }
// key points the pass reads: s_0 .. s_{N-2}
PLK_FK_HD uint64_t fk_key_points_needed(uint32_t log_n) { return ((uint64_t)1 << log_n) - 1; }
PLK_FK_HD bool fk_key_ok(uint32_t log_n, uint64_t resident) { return resident >= fk_key_points_needed(log_n); }

// the key's transform that a context keeps: 2N points, XYZZ on the 29-bit layer
PLK_FK_HD size_t fk_key_transform_bytes(uint32_t log_n) { return ((size_t)2 << log_n) * FK_XYZZW_BYTES; }
// scratch of one call: [ u: 2N XYZZ points | c: 2N Fr | coefficients: N Fr (PLK_KZG_VALUES only) ]
struct FkScratch { size_t u_off, c_off, coeff_off, bytes; };
PLK_FK_HD FkScratch fk_scratch(uint32_t log_n, bool values) {
    const size_t n = (size_t)1 << log_n;
    FkScratch s;
    s.u_off = 0;
    s.c_off = 2 * n * FK_XYZZW_BYTES;
    s.coeff_off = s.c_off + 2 * n * FK_FR_BYTES;
    s.bytes = s.coeff_off + (values ? n * FK_FR_BYTES : 0);
    return s;
}

// ---- a batch: `count` polynomials of N = 2^log_n under one key (plk_kzg_open_all_batch_dev), `count` transforms per stage launch (g1ntt.hip).
// The polynomial is the SLOW index of every launch; the transforms' first points lie `stride` points apart (2N in the scratch of the openings,
// N in the public G1 batch).  Every flattened index stays inside 32 bits: a launch covers at most 2^26 points.
constexpr uint32_t FK_BATCH_LOG_POINTS = 26;                       // g1ntt's limit, applied to the whole launch
// count transforms of 2^log_points points in one launch
PLK_FK_HD bool fk_batch_points_ok(uint32_t count, uint32_t log_points) {
    return count >= 1 && log_points <= FK_BATCH_LOG_POINTS && ((uint64_t)count << log_points) <= ((uint64_t)1 << FK_BATCH_LOG_POINTS);
}
// count polynomials of 2^log_n: the 2N-point transforms of all of them are one launch
PLK_FK_HD bool fk_batch_ok(uint32_t count, uint32_t log_n) { return fk_size_ok(log_n) && fk_batch_points_ok(count, log_n + 1); }
// scratch of a batch call: [ u: count x 2N XYZZ points | c: count x 2N Fr | coefficients: count x N Fr (PLK_KZG_VALUES only) ]; fk_scratch for count = 1
PLK_FK_HD FkScratch fk_batch_scratch(uint32_t count, uint32_t log_n, bool values) {
    const size_t n = (size_t)1 << log_n;
    FkScratch s;
    s.u_off = 0;
    s.c_off = count * 2 * n * FK_XYZZW_BYTES;
    s.coeff_off = s.c_off + count * 2 * n * FK_FR_BYTES;
    s.bytes = s.coeff_off + (values ? count * n * FK_FR_BYTES : 0);
    return s;
}
// flattened butterfly g < count * 2^(log_n - 1) of a stage launch over transforms of 2^log_n points (log_n >= 1) -> (transform, butterfly in it)
struct FkButterfly { uint32_t poly, j; };
PLK_FK_HD FkButterfly fk_batch_butterfly(uint32_t log_n, uint32_t g) {
    FkButterfly b;
    b.poly = g >> (log_n - 1);
    b.j = g & ((1u << (log_n - 1)) - 1);
    return b;
}
// butterfly j < 2^(log_n - 1) of stage s < log_n (half-size 2^s) -> its two points i0 < i1 inside the transform and its twiddle position jl.
// In the early stages of a transform of 256 points or more the position is the slow index, so whole waves share a twiddle (g1ntt_stage).
struct FkPair { uint32_t i0, i1, jl; };
PLK_FK_HD FkPair fk_stage_pair(uint32_t log_n, uint32_t s, uint32_t j) {
    const uint32_t h = 1u << s;
    uint32_t jl, jh;
    if (s < 6 && log_n >= 8) { jl = j >> (log_n - 1 - s); jh = j & ((1u << (log_n - 1 - s)) - 1); }
    else { jl = j & (h - 1); jh = j >> s; }
    FkPair p;
    p.i0 = (jh << (s + 1)) | jl;
    p.i1 = p.i0 + h;
    p.jl = jl;
    return p;
}
// flattened point p < count * 2^log_n (the first 2^log_n of every transform, dense) -> where it lies among transforms `stride` points apart
PLK_FK_HD uint32_t fk_batch_point(uint32_t log_n, uint32_t stride, uint32_t p) { return (p >> log_n) * stride + (p & ((1u << log_n) - 1)); }

}  // namespace plk
