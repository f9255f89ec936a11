// Many multi-point openings verified on the device, each on its own (kzg_multi_verify.hip): what a pass holds and where, as plain
// functions of the shape.  Host-compilable like kzg_multi_plan.h — <stdint.h> alone, no HIP, no environment — so a stand-alone program
// checks it against numbers it is handed (tests/host/kzg_multi_verify_check.hip); every function is constexpr, which is also what lets the
// kernels call the same text.  NO COUNTERPART IN THE REFERENCE: bellman's kate_commitment opens at one point per call.
//
// One shape (count polynomials, npoints points, the sets) serves the whole batch.  Per opening a pass keeps
//     count + 3 scalars      c_0 .. c_{count-1}, -sum c_i r_i(u), -Z_T(u), u       32 B each (Montgomery)
//     count + 3 products     scalar x (C_0 .. C_{count-1}, G, W, W')               144 B each (XyzzW)
//     pairs running products of the differences t_j - t_l, j < l, then their inverses   32 B each
//     A and B                the pairing kernel's input                            64 B each
//     two bytes              the pairing kernel's verdict and the front's state
// and the arrays stand behind one another, each 16-byte aligned.
#pragma once
#include <stdint.h>

namespace plk {
namespace host {

constexpr uint32_t KMV_MAX_OPEN = 32, KMV_MAX_POINTS = 8;             // KM_MAX_OPEN, KM_MAX_POINTS (kzg_multi_plan.h)
constexpr uint32_t KMV_FR_BYTES = 32, KMV_AFFINE_BYTES = 64, KMV_XYZZW_BYTES = 144;
constexpr uint32_t KMV_BLOCK = 256;                                   // lanes of a workgroup of every kernel; G1NTT_THREADS for the terms
constexpr uint64_t KMV_PASS_MAX = 1u << 16;                           // openings per pass, at most (the pairing kernel's pass)
constexpr uint64_t KMV_PASS_BYTES = 64ull << 20;                      // a pass's buffer, at most
constexpr uint32_t KMV_STATE_GOES_ON = 1, KMV_STATE_MALFORMED = 2;    // FRONT_GOES_ON, FRONT_MALFORMED (verify_front_dev.h); no state 0 here

constexpr uint32_t kmv_terms(uint32_t count) { return count + 3; }
constexpr uint32_t kmv_pairs(uint32_t npoints) { return npoints * (npoints - 1) / 2; }
// the place of t_j - t_l, j < l, among the pairs: (0,1) (0,2) .. (0,p-1) (1,2) ..
constexpr uint32_t kmv_pair(uint32_t j, uint32_t l, uint32_t npoints) { return j * npoints - j * (j + 1) / 2 + (l - j - 1); }

constexpr uint64_t kmv_bytes_per_opening(uint32_t count, uint32_t npoints) {
    return (uint64_t)kmv_terms(count) * (KMV_FR_BYTES + KMV_XYZZW_BYTES) + (uint64_t)kmv_pairs(npoints) * KMV_FR_BYTES + 2 * KMV_AFFINE_BYTES + 2;
}
// openings per pass: a multiple of 256, at most 2^16, the pass's buffer at most 64 MiB
constexpr uint64_t kmv_pass(uint32_t count, uint32_t npoints) {
    const uint64_t fit = KMV_PASS_BYTES / kmv_bytes_per_opening(count, npoints) / KMV_BLOCK * KMV_BLOCK;
    return fit < KMV_PASS_MAX ? fit : KMV_PASS_MAX;
}

// byte offsets of the arrays of a pass of m openings (m <= kmv_pass); every one a multiple of 16
struct KmvLayout { uint64_t scalars, products, run, a, b, verdict, state, total; };
constexpr uint64_t kmv_pad16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }
constexpr KmvLayout kmv_layout(uint32_t count, uint32_t npoints, uint64_t m) {
    KmvLayout L{};
    L.scalars = 0;
    L.products = L.scalars + m * kmv_terms(count) * KMV_FR_BYTES;
    L.run = L.products + m * kmv_terms(count) * KMV_XYZZW_BYTES;
    L.a = L.run + m * kmv_pairs(npoints) * KMV_FR_BYTES;
    L.b = L.a + m * KMV_AFFINE_BYTES;
    L.verdict = L.b + m * KMV_AFFINE_BYTES;
    L.state = L.verdict + kmv_pad16(m);
    L.total = L.state + kmv_pad16(m);
    return L;
}
// the front on its own (plk_kzg_verify_multi_front_dev) keeps the running products alone; scalars and states go to the caller
constexpr uint64_t kmv_front_bytes(uint32_t npoints, uint64_t m) { return m * kmv_pairs(npoints) * KMV_FR_BYTES; }

// (opening, term) <-> lane of the term kernel: an opening's terms are neighbours, so a wave shares its scalars' cache lines
constexpr uint64_t kmv_lanes(uint64_t openings, uint32_t count) { return openings * kmv_terms(count); }
constexpr uint32_t kmv_lane(uint32_t opening, uint32_t term, uint32_t count) { return opening * kmv_terms(count) + term; }
constexpr uint32_t kmv_lane_opening(uint32_t lane, uint32_t count) { return lane / kmv_terms(count); }
constexpr uint32_t kmv_lane_term(uint32_t lane, uint32_t count) { return lane % kmv_terms(count); }
constexpr uint32_t kmv_blocks(uint64_t lanes) { return (uint32_t)((lanes + KMV_BLOCK - 1) / KMV_BLOCK); }
// which base a term multiplies: its commitment, the generator, W, W'
enum KmvBase : uint32_t { KMV_BASE_COMMITMENT = 0, KMV_BASE_G = 1, KMV_BASE_W = 2, KMV_BASE_W2 = 3 };
constexpr uint32_t kmv_term_base(uint32_t term, uint32_t count) { return term < count ? (uint32_t)KMV_BASE_COMMITMENT : term - count + 1; }

static_assert(kmv_pass(32, 8) * kmv_bytes_per_opening(32, 8) <= KMV_PASS_BYTES && kmv_pass(32, 8) % KMV_BLOCK == 0 && kmv_pass(32, 8) > 0, "the largest shape fits");
static_assert(kmv_pass(1, 1) == KMV_PASS_MAX, "the smallest shape is capped by the pairing kernel's pass");
static_assert(kmv_lanes(KMV_PASS_MAX, 1) < (1ull << 32) && kmv_lanes(kmv_pass(32, 8), 32) < (1ull << 32), "a pass's lanes fit 32 bits");

}  // namespace host
}  // namespace plk
