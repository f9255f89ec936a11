// Declarations shared by msm.hip (recoding, partition, bucket reduction, drivers) and msm_accumulate.hip (kernel A, the
// dominant kernel of the library, a translation unit of its own since round 4 so that it can be compiled with the scheduling
// strategy that suits it — see msm_accumulate.hip).
#pragma once
#include "ctx.h"
#include "ec_dev.h"
#include "ec29_dev.h"
#include "msm_plan.h"

namespace plk {

// Every dispatch constant (MSM_THREADS, FINE_BITS, CHUNK, MSM_MAX_BATCH, RC_WINDOWS, ...) and MsmParams: msm_plan.h, which is host-only; here is what
// needs device types.
static_assert(sizeof(Fr) == MSM_BYTES_FR && sizeof(G1Affine) == MSM_BYTES_AFFINE && sizeof(G1Xyzz) == MSM_BYTES_XYZZ && sizeof(XyzzW) == MSM_BYTES_XYZZW,
              "msm_plan.h sizes the buffers with these");

struct ScalarSet { const Fr *v[MSM_MAX_BATCH]; };

// ---- scalar recoding shared by msm.hip (fused pre-phase) and msm_small.hip (host-callable too: tests/host/arith_kat.hip runs them on the CPU and on the GPU)
PLK_HD uint32_t extract_bits(const uint32_t *k, uint32_t pos, uint32_t c) {
    uint32_t limb = pos >> 5, off = pos & 31;
    if (limb >= 8) return 0;
    uint64_t v = k[limb];
    if (limb + 1 < 8) v |= (uint64_t)k[limb + 1] << 32;
    return (uint32_t)(v >> off) & ((1u << c) - 1);
}
// the signed digits of msm_digits for c = 17, 15 windows, in registers: d[w] in [-2^16, 2^16], top window unsigned
PLK_HD void recode17(const Fr &k, int32_t (&d)[RC_WINDOWS]) {
    uint32_t carry = 0;
#pragma unroll
    for (uint32_t w = 0; w < RC_WINDOWS; w++) {
        const uint32_t v = extract_bits(k.l, w * 17, 17) + carry;
        if (v >= (1u << 16) && w + 1 < RC_WINDOWS) { d[w] = (int32_t)v - (1 << 17); carry = 1; } else { d[w] = (int32_t)v; carry = 0; }
    }
}
// the same digits from the nine 29-bit limbs of the canonical scalar (fr_canonical_w), without packing it into words first: window w is bits
// 17w .. 17w+16 of the same integer, which lie in limb 17w / 29 and, where they cross its end, the next one.  recode17_w(fr_canonical_w(k))
// == recode17(to_canonical(k)) digit for digit (tests/host/field29_pairs_check.hip).
PLK_HD void recode17_w(const FrW9 &k, int32_t (&d)[RC_WINDOWS]) {
    uint32_t carry = 0;
#pragma unroll
    for (uint32_t w = 0; w < RC_WINDOWS; w++) {
        const uint32_t limb = (w * 17) / 29, off = (w * 17) % 29;
        uint32_t v = k.l[limb] >> off;
        if (off + 17 > 29 && limb + 1 < 9) v |= k.l[limb + 1] << (29 - off);
        v = (v & ((1u << 17) - 1)) + carry;
        if (v >= (1u << 16) && w + 1 < RC_WINDOWS) { d[w] = (int32_t)v - (1 << 17); carry = 1; } else { d[w] = (int32_t)v; carry = 0; }
    }
}

// Per-task output of kernel A: 128 PRIMARY slots (a bucket whose run lies inside one lane's slice), and per
// lane one HEAD slot (its first run continues a bucket begun by an earlier lane) and one TAIL slot (its last
// run is continued by a later lane).  Which slots are live follows from the bucket offsets alone.
template <uint32_t FB> struct Shape {
    static constexpr uint32_t FINE = 1u << FB;
    static constexpr uint32_t SLOT_PRIMARY = 0, SLOT_HEAD = FINE, SLOT_TAIL = FINE + MSM_THREADS, SLOTS_PER_TASK = FINE + 2 * MSM_THREADS;
    static constexpr uint32_t META_PER_TASK = FINE + 2;   // start[0..FINE] and the entry count
};

// bit 31 of a task's entry count in its meta block: the task's buckets were accumulated by the lanes that own them (msm_accumulate<.., OWNED>): one PRIMARY
// sum per bucket, no HEAD / TAIL pieces
constexpr uint32_t TASK_OWNED_BIT = 0x80000000u;

// kernel A (msm_accumulate.hip): one workgroup per task of 2^FINE_BITS buckets; variant 0 = the plain kernel, variant 2 = the build that lets a
// task's lanes own its buckets when they are evenly filled (commitments of <= 2^16 terms).  Variant 1 (a 512-register, one-wave-per-SIMD
// build kept for measurements) is retired; the numbers stay as they are because plk_msm_last_shape reports them.
// no_inf: the table holds no point at infinity (msm.hip: ensure_base_table) — variant 0 then runs the instantiation without the is_inf(q) test.
int32_t msm_accumulate_prepare();                                   // dynamic-LDS attributes, once per process
void msm_accumulate_launch(int variant, bool no_inf, uint32_t max_tasks, hipStream_t stream, const G1Affine *bases, const uint32_t *entries,
                           const uint32_t *bin_start, const uint32_t *task_start, XyzzW *partials, uint32_t *task_meta, const MsmParams &p);

}  // namespace plk
