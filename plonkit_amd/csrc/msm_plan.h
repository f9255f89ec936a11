// Which kernels a commitment is given: every dispatch decision of the MSM (msm.hip, msm_accumulate.hip, msm_small.hip) and every constant
// it rests on, as pure functions of integers.  Host code only: no HIP include, no environment, no context — so a stand-alone program can
// check the whole dispatch in milliseconds (tests/host/msm_plan_check.cpp, tests/test_msm_plan_host.py), where the GPU table of
// tests/test_gpu_msm_shapes.py needs keys of gigabytes.
//   msm_plan_pass      one pass of the kernels (msm_enqueue_batch): path, window bits, table copies, pre-phase, accumulate variant,
//                      reduction lanes, MsmParams, grids and buffer sizes
//   msm_plan_pipeline  its bucket-pipeline half on its own
//   msm_plan_fallback  the re-run of a short commitment whose bucket lists overflowed (msm_finish_batch)
//   msm_plan_call      one call of plk_msm_g1 / _dev / _partial_dev: piece length, pieces in flight, number of pieces
//   msm_plan_bases_pass / msm_plan_bases_call   the same two for caller-supplied bases (plk_msm_g1_bases*): no key, no table
//   "the bucket schedule"   the integer rules INSIDE the kernels (slices of a bin, entries per lane, owned tasks, the span of a bucket, folding
//                      a bin's tasks): constexpr, called by the kernels and by tests/host/msm_bucket_cases_check.cpp alike
// msm.hip's host side computes a plan, then reserves, launches and records; it decides nothing.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/plonkit_amd.h"

namespace plk {

// ---------------------------------------------------------------------------------------------- constants
constexpr int MSM_THREADS = 256;
// Buckets per accumulate workgroup = 2^FB ("fine" part of the bucket index; the coarse part selects the bin).  The kernels
// keep FB as a template parameter; one shape is compiled:
//   FB = 6: 64 buckets per task.  At c = 17 that is 1024 coarse bins of ~15 K entries at 2^20 terms = ONE task per bin,
//           so every bucket is reduced once (65 K task-buckets) — the bucket reduction (msm_task_reduce) is not a latency
//           detail: in VALU work it was 38 % of the accumulation (992 waves x 37 dependent full additions of 14 products
//           against 15.7 M mixed additions of 9.3), and it shares the GPU with the next commitment's accumulation.
//   (FB = 7, 128 buckets per task and two tasks per bin at 2^20 terms, was the round-1 shape; no window width in use needs it.)
constexpr uint32_t FINE_BITS = 6;
constexpr uint32_t CHUNK = 16384;                // entries per accumulate workgroup (sorted in 64 KB of LDS; two workgroups per CU)
constexpr uint32_t DIGIT_CHUNK = 16384;            // scalars per partition workgroup (per window): 64 KB of LDS staging
constexpr uint32_t TASK_MAX = CHUNK;
                   // per-chunk bucket population handled cooperatively

constexpr uint32_t MSM_MAX_BATCH = 8;              // commitments sharing one pass over the same bases
constexpr uint32_t MSM_SLOTS = 3;                  // commitments (or batches) in flight on one context (ctx.h: MsmSlot), and the pieces of a long one

constexpr int RC_WINDOWS = 15;                      // 17-bit windows over the 254-bit scalars
// fused recoding (msm_recode_count / msm_recode_scatter, msm.hip): the workgroup of the scatter pass takes RC_SCALARS scalars x 15 windows;
// RC_COUNT_PER scalars per thread of the count pass keep the global atomics at one per (workgroup, bin) for 4096 scalars
constexpr int RC_THREADS = 1024, RC_SCALARS = 1024;
constexpr int RC_COUNT_PER = 4;
static_assert(RC_WINDOWS == 254 / 17 + 1, "the fused path is the c = 17 shape");

// The SRS is a fixed base: copy k of the table holds 2^(17k) * P_i (msm.hip: ensure_base_table).
constexpr uint32_t COPY_SHIFT = 17, MAX_COPIES = 15;    // 15 windows of 17 bits cover the 254-bit scalars

// fewer terms than this without the table's copies: one double-and-add per term (msm_naive), block sums to the host
constexpr uint64_t MSM_NAIVE_BELOW = 4096;
// terms up to which a commitment takes the short path (msm_small.hip): 2^15 (measured, one at a time: 2^14 terms 0.27 against 0.62 ms, 2^15 0.35 against
// 0.53, 2^16 0.52 against 0.54; a proof at the 2^15 domain 3.25 against 3.40 ms; at 2^16 a batch of two is SLOWER on this path — a proof 3.76 against
// 3.56 ms — and a batch of four much slower: 4.85)
constexpr uint64_t MSM_SMALL_MAX = 1ull << 15;
// key size up to which the 15 copies are cheap enough to build for a short commitment of fewer than 4096 terms (<= 2^21 points: 80 ms once per key)
constexpr uint64_t MSM_SMALL_CHEAP_KEY = 1ull << 21;
constexpr uint32_t SM_PLANES_HOST = 17;            // plane sums per commitment that the short path leaves for the host (msm_small.hip: SM_PLANES)
// terms up to which msm_accumulate is launched in the build whose lanes own the buckets of an evenly filled task (msm_accumulate.hip)
constexpr uint64_t MSM_OWNED_MAX = 1ull << 16;
// one pass of the kernels takes at most 2^24 terms: (copy, index) share the 24-bit field of a bucket entry
constexpr uint64_t MSM_PASS_MAX_TERMS = 1ull << 24;
// From 2^23 terms on, ONE commitment is better run as 2^20-term pieces over successive SRS ranges, three pieces in flight: the
// digit / partition kernels and the bucket reduction of a piece then overlap the accumulation of its neighbours, which a single
// pass cannot do with itself (2^24 terms: 21.8 ms against 24.0 in one pass; at 2^22 the pieces do not pay: 6.5 against 6.15 ms,
// profiles/r02_msm_three_in_flight_ab.txt).  Only with the table of shifted copies: an SRS of more than 2^25 points has none
// (it would exceed 32 GiB), a 2^20-term piece then runs 19 windows instead of 15 and a 2^26-gate proof got 40 % SLOWER that way.
constexpr uint64_t MSM_PIPELINE_MIN_TERMS = 1ull << 23, MSM_PIPELINE_PIECE = 1ull << 20;

// window reduction (msm_window_sums_quad, msm.hip): per bucket set role 0 and the LAST role are the sums of the S_t (bins below / from
// nbins / 2), roles 1..8 the bit sums G_0..G_7, roles 9.. F_1.. — what the host fold of msm_finish_batch reads
constexpr uint32_t THREADS_LOG = 8;
static_assert((1u << THREADS_LOG) == MSM_THREADS, "THREADS_LOG");
constexpr uint32_t WS_BIT_ROLES = THREADS_LOG, WS_FIRST_F_ROLE = 1 + WS_BIT_ROLES;

// ---------------------------------------------------------------------------------------------- the bucket schedule
// The integer rules that decide which code a bucket takes between the scan of the bins and the bucket reduction.  constexpr, so the kernels
// (msm_scan_bins, msm_accumulate, msm_fold_hot, msm_task_reduce, msm_task_reduce_quad, msm_bin_fold) and a stand-alone host program
// (tests/host/msm_bucket_cases_check.cpp) evaluate the SAME text: a threshold has one copy, and a case table that sits on it is checked
// on the CPU (tests/test_msm_bucket_cases_host.py) before the GPU runs it (tests/test_gpu_msm_bucket_edges.py).
//
// (MSM_RULE: inlined before anything else is optimised, so a kernel that calls a rule compiles to the instructions of the expression written out.)
#define MSM_RULE constexpr __attribute__((always_inline))
// A bin of `count` entries becomes k = ceil(count / TASK_MAX) tasks (msm_scan_bins), cut into k EQUAL slices of ceil(count / k) entries, the
// last one shorter (head of msm_accumulate).  [bs, be) is the bin's range in the entry array.
MSM_RULE uint32_t msm_bin_tasks(uint32_t count) { return (count + TASK_MAX - 1) / TASK_MAX; }
MSM_RULE uint32_t msm_slice_per(uint32_t count, uint32_t k) { return (count + k - 1) / k; }
MSM_RULE uint32_t msm_slice_begin(uint32_t bs, uint32_t be, uint32_t per, uint32_t slice) { return bs + slice * per < be ? bs + slice * per : be; }
MSM_RULE uint32_t msm_slice_end(uint32_t s, uint32_t be, uint32_t per) { return (s + per < be) ? s + per : be; }
MSM_RULE uint32_t msm_slice_len(uint32_t count, uint32_t k, uint32_t slice) {
    return msm_slice_end(msm_slice_begin(0, count, msm_slice_per(count, k), slice), count, msm_slice_per(count, k)) - msm_slice_begin(0, count, msm_slice_per(count, k), slice);
}
// The sorted slice of nc entries is cut into MSM_THREADS equal pieces of mu entries: lane `tid` takes [lo, hi); lanes with lo >= hi leave
// early and the last live lane has a short piece.  (msm_fold_hot, msm_task_reduce and msm_task_reduce_quad recompute mu from the task's
// meta with msm_lane_entries' expression written out — see the note above bucket_span in msm.hip; a change here is a change there.)
MSM_RULE uint32_t msm_lane_entries(uint32_t nc) { return (nc + MSM_THREADS - 1) / MSM_THREADS; }
MSM_RULE uint32_t msm_lane_lo(uint32_t tid, uint32_t mu, uint32_t nc) { return tid * mu < nc ? tid * mu : nc; }
MSM_RULE uint32_t msm_lane_hi(uint32_t lo, uint32_t mu, uint32_t nc) { return lo + mu < nc ? lo + mu : nc; }
// A task of the owned build (commitments of <= MSM_OWNED_MAX terms) is OWNED — four lanes per bucket, one PRIMARY sum per bucket,
// TASK_OWNED_BIT in its meta — iff its fullest bucket holds at most MSM_OWNED_SPAN * mu + MSM_OWNED_SLACK entries.
constexpr uint32_t MSM_OWNED_SPAN = 8, MSM_OWNED_SLACK = 24;
MSM_RULE bool msm_task_owned(uint32_t max_cnt, uint32_t mu) { return max_cnt <= MSM_OWNED_SPAN * mu + MSM_OWNED_SLACK; }
// A bucket [s0, e0) of the sorted slice, s0 < e0, lies in the pieces of lanes tf .. tl.  tf == tl: one PRIMARY sum.  Otherwise the TAIL of
// lane tf and the HEADs of lanes tf + 1 .. tl, which the reduction walks when tl - tf <= HOT_SPAN and msm_fold_hot folds into the bucket's
// PRIMARY slot beforehand when the span is larger.
constexpr uint32_t HOT_SPAN = 8;
MSM_RULE uint32_t msm_bucket_first_lane(uint32_t s0, uint32_t mu) { return s0 / mu; }
MSM_RULE uint32_t msm_bucket_last_lane(uint32_t e0, uint32_t mu) { return (e0 - 1) / mu; }
MSM_RULE uint32_t msm_bucket_span(uint32_t s0, uint32_t e0, uint32_t mu) { return e0 > s0 ? msm_bucket_last_lane(e0, mu) - msm_bucket_first_lane(s0, mu) : 0; }
MSM_RULE bool msm_span_folded(uint32_t span) { return span > HOT_SPAN; }
enum : uint32_t { MSM_BUCKET_EMPTY = 0, MSM_BUCKET_PRIMARY = 1, MSM_BUCKET_WALKED = 2, MSM_BUCKET_FOLDED = 3 };
MSM_RULE uint32_t msm_bucket_class(uint32_t s0, uint32_t e0, uint32_t mu) {
    return e0 <= s0 ? MSM_BUCKET_EMPTY
                    : msm_bucket_first_lane(s0, mu) == msm_bucket_last_lane(e0, mu) ? MSM_BUCKET_PRIMARY
                    : msm_span_folded(msm_bucket_span(s0, e0, mu)) ? MSM_BUCKET_FOLDED : MSM_BUCKET_WALKED;
}
// msm_bin_fold adds up the task sums of a bin of MORE than BIN_FOLD_MIN tasks; smaller bins are left to msm_window_sums_quad.
constexpr uint32_t BIN_FOLD_MIN = 4;
MSM_RULE bool msm_bin_folded(uint32_t tasks) { return tasks > BIN_FOLD_MIN; }

// record sizes of the device types the buffers hold (msm_shape.h asserts them against the types)
constexpr size_t MSM_BYTES_FR = 32, MSM_BYTES_AFFINE = 64, MSM_BYTES_XYZZ = 128, MSM_BYTES_XYZZW = 144;

// All 15 copies or none: a commitment that can only address 5 or 3 of them ((copy, index) must fit the 24-bit
// field of an entry) uses every 3rd or 5th copy, so the full table serves every size.
constexpr uint64_t MSM_TABLE_CAP_BYTES = 32ull << 30;
inline uint32_t table_copies_for(uint64_t srs_n) {           // the table may take up to 32 GiB of the 288 GB
    return (uint64_t)MAX_COPIES * srs_n * MSM_BYTES_AFFINE <= MSM_TABLE_CAP_BYTES ? MAX_COPIES : 1;
}

// Window widths are chosen among those whose top window still has many bits (254 = 19*13 + 7 = 16*15 + 14 = 15*16 + 14):
// a top window of 1-2 bits would put every term into two or three buckets of a single bin.
inline uint32_t pick_window_bits(uint64_t n, bool have_table) {
    // with the table of shifted copies every size is best served by 17-bit windows and one bucket set (measured
    // against 13/15-bit windows without it: 2^12 0.50 vs 0.64 ms, 2^14 0.58 vs 0.95, 2^16 0.62 vs 0.98, 2^18 0.87 vs 1.12)
    if (have_table) return COPY_SHIFT;
    if (n < (1u << 17)) return 13;
    if (n < (1u << 19)) return 15;
    return 17;                                                // 15 windows; 2^16 buckets = 512 coarse bins x 128
}

// per-task output of kernel A (msm_shape.h: Shape): PRIMARY, HEAD and TAIL slots; bucket offsets and the entry count
inline uint32_t slots_per_task(uint32_t fb) { return (1u << fb) + 2 * MSM_THREADS; }
inline uint32_t meta_per_task(uint32_t fb) { return (1u << fb) + 2; }

struct MsmParams {
    uint32_t n;
    uint32_t c;               // window bits
    uint32_t windows;         // W per commitment
    uint32_t fine_bits;       // FB: buckets per accumulate task = 2^FB
    uint32_t coarse_bits;     // c - 1 - fine_bits
    uint32_t nbins;           // 1 << coarse_bits
    uint32_t batch;           // number of scalar vectors (same n, same bases); "global window" = m * W + w
    // Shifted copies of the bases (fixed-base precomputation): window w = j*groups + g takes its points from
    // copy j*groups of the table (2^(16*j*groups) * P_i) and drops them into bucket set g, so only `groups`
    // bucket sets have to be reduced and only c*groups doublings are left for the host Horner.
    uint32_t groups;          // bucket sets per commitment (= windows when there is one copy)
    uint32_t nbits;           // entry index = (j << nbits) | i
    uint32_t copy_stride;     // points between table copies j and j+1 (= groups * srs_n)
};

// ---------------------------------------------------------------------------------------------- the plan of one pass
enum : uint32_t { MSM_RUN_NOTHING = 0,      // zero terms
                  MSM_RUN_NAIVE = 1,        // msm_naive: `grid_naive` block sums per commitment for the host
                  MSM_RUN_SHORT = 2,        // msm_small.hip: SM_PLANES_HOST plane sums per commitment and the overflow flag
                  MSM_RUN_PIPELINE = 3 };   // recode / partition, accumulate, bucket reduction: `roles` points per bucket set

// (64-bit members first, an even number of 32-bit ones: no padding, so equal plans are equal bytes)
struct MsmPlan {
    plk_msm_shape shape;                    // what plk_msm_last_shape reports; path SHORT_FALLBACK only from msm_plan_fallback
    uint64_t terms, srs_n;
    // RUN_PIPELINE (RUN_NAIVE: bytes_d and bytes_pinned; RUN_SHORT: bytes_pinned):
    size_t bytes_a;                         // hist / cursor, bin_start, task_start
    size_t bytes_b;                         // entries
    size_t bytes_c;                         // per-task (S, T) + bucket offsets
    size_t bytes_d;                         // per bucket set: sum S, G_0..G_7, F_1..F_3 (naive: the block sums)
    size_t bytes_e;                         // lane partial sums
    size_t bytes_f;                         // canonical scalars, pass 1 -> pass 2 (fused), or the digit array
    size_t bytes_pinned;                    // what the host fold reads
    size_t lds_recode_scatter, lds_partition_count, lds_partition_scatter;
    MsmParams p;                            // RUN_PIPELINE and RUN_SHORT (whose re-run keeps c, nbits and the copies); otherwise n, batch, nbits only
    uint32_t run;                           // MSM_RUN_*
    uint32_t table_request;                 // copies to ask ensure_base_table for (0: the re-run at the finish asks for nothing)
    uint32_t copies;                        // copies the commitment addresses
    uint32_t total_sets, total_bins, total_windows, max_tasks;
    uint32_t roles;                         // points per bucket set left for the host: S (bins below nbins / 2), G_0..G_7, F_1 .., S (bins from nbins / 2)
    uint32_t grid_recode_count, grid_recode_scatter;        // fused pre-phase
    uint32_t grid_digits, grid_partition;                   // pre-phase through the digit array (x batch, x total_windows)
    uint32_t grid_reduce, grid_reduce_quad, grid_bin_fold;  // msm_fold_hot / msm_task_reduce, msm_task_reduce_quad, msm_bin_fold
    uint32_t grid_naive;                                    // msm_naive, per commitment
};
static_assert(sizeof(MsmPlan) == sizeof(plk_msm_shape) + 2 * 8 + 10 * sizeof(size_t) + sizeof(MsmParams) + 16 * 4, "MsmPlan has padding");

inline uint32_t msm_index_bits(uint64_t terms) {              // entry index = (copy << nbits) | i
    uint32_t nbits = 1;
    while ((1ull << nbits) < terms) nbits++;
    return nbits;
}

inline MsmPlan msm_plan_nothing(uint64_t terms, uint32_t batch, uint64_t srs_n) {
    MsmPlan P{};
    P.shape.path = PLK_MSM_PATH_EMPTY; P.shape.batch = batch; P.shape.pieces = 1; P.shape.piece_terms = terms;
    P.terms = terms; P.srs_n = srs_n;
    P.p.n = (uint32_t)terms; P.p.batch = batch; P.p.nbits = msm_index_bits(terms);
    P.run = MSM_RUN_NOTHING;
    P.copies = 1;
    return P;
}

// fewer than 4096 terms without the table's copies: one double-and-add per term (msm_naive), block sums to the host
inline MsmPlan msm_plan_naive(uint64_t terms, uint32_t batch, uint64_t srs_n) {
    MsmPlan P = msm_plan_nothing(terms, batch, srs_n);
    P.run = MSM_RUN_NAIVE;
    P.shape.path = PLK_MSM_PATH_NAIVE; P.shape.table_copies = 1;
    P.grid_naive = (uint32_t)((terms + MSM_THREADS - 1) / MSM_THREADS);
    P.bytes_d = P.bytes_pinned = (size_t)batch * P.grid_naive * MSM_BYTES_XYZZ;
    return P;
}

inline MsmParams msm_params(uint64_t terms, uint32_t batch, uint64_t srs_n, uint32_t copies, uint32_t c_bits, uint32_t nbits) {
    MsmParams p;
    p.n = (uint32_t)terms;
    p.c = c_bits;
    p.windows = 254 / p.c + 1;
    p.groups = p.windows / copies;                            // copies > 1 only for c = 17: 15 windows, copies | 15
    p.nbits = nbits;
    p.copy_stride = copies > 1 ? (uint32_t)(p.groups * srs_n) : 0;
    p.fine_bits = FINE_BITS;
    p.coarse_bits = p.c - 1 - p.fine_bits;                    // c is 13, 15 or 17: at most the 1024 coarse bins msm_window_sums_quad serves
    p.nbins = 1u << p.coarse_bits;
    p.batch = batch;
    return p;
}

// the 2^20-shaped pipeline (recode / partition, accumulate, bucket reduction) for one batch.  Callable on its own: msm_plan_fallback runs
// it at the finish with the copies, window bits and index bits chosen at the enqueue.
inline MsmPlan msm_plan_pipeline(uint64_t terms, uint32_t batch, uint64_t srs_n, uint32_t copies, uint32_t c_bits, uint32_t nbits,
                                 bool others_in_flight, bool fused_allowed) {
    MsmPlan P = msm_plan_nothing(terms, batch, srs_n);
    P.run = MSM_RUN_PIPELINE;
    P.copies = copies;
    const MsmParams p = P.p = msm_params(terms, batch, srs_n, copies, c_bits, nbits);
    const uint64_t n = terms;
    const uint32_t total_sets = batch * p.groups, total_bins = total_sets * p.nbins, total_windows = batch * p.windows;
    const uint32_t max_tasks = total_bins + (uint32_t)(((uint64_t)total_windows * n) / TASK_MAX) + 1;
    P.total_sets = total_sets; P.total_bins = total_bins; P.total_windows = total_windows; P.max_tasks = max_tasks;
    const uint32_t META_PER_TASK = meta_per_task(p.fine_bits), SLOTS_PER_TASK = slots_per_task(p.fine_bits);
    P.bytes_a = (size_t)(3 * total_bins + 4) * sizeof(uint32_t);
    P.bytes_b = (size_t)total_windows * n * sizeof(uint32_t);
    P.bytes_c = (size_t)max_tasks * 2 * MSM_BYTES_XYZZW + (size_t)max_tasks * META_PER_TASK * 4;
    P.bytes_e = (size_t)max_tasks * SLOTS_PER_TASK * MSM_BYTES_XYZZW;
    P.bytes_d = (size_t)13 * total_sets * MSM_BYTES_XYZZ;
    // pre-phase.  One bucket set per commitment (the 2^20 shape): digits never leave the registers (msm_recode_count / _scatter);
    // otherwise, or when the caller does not allow it (A/B knob), the three-launch pre-phase through the digit array
    const uint32_t prephase = (fused_allowed && p.groups == 1 && p.c == 17 && p.windows == RC_WINDOWS && p.nbins <= 1024) ? 1u : 2u;
    if (prephase == 1) {
        P.grid_recode_count = (uint32_t)((n + (uint64_t)RC_THREADS * RC_COUNT_PER - 1) / ((uint64_t)RC_THREADS * RC_COUNT_PER));
        P.grid_recode_scatter = (uint32_t)((n + RC_SCALARS - 1) / RC_SCALARS);
        P.lds_recode_scatter = (size_t)(3 * p.nbins + 1 + RC_SCALARS * RC_WINDOWS) * sizeof(uint32_t);
        P.bytes_f = (size_t)batch * n * MSM_BYTES_FR;
    } else {
        P.grid_digits = (uint32_t)((n + MSM_THREADS - 1) / MSM_THREADS);
        P.grid_partition = (uint32_t)((n + DIGIT_CHUNK - 1) / DIGIT_CHUNK);
        P.lds_partition_count = (size_t)p.nbins * sizeof(uint32_t);
        P.lds_partition_scatter = (size_t)(3 * p.nbins + 1 + DIGIT_CHUNK) * sizeof(uint32_t);
        P.bytes_f = (size_t)total_windows * n * sizeof(int32_t);
    }
    // commitments of <= 2^16 terms: the build whose lanes own the buckets of an evenly filled task (msm_accumulate.hip)
    const uint32_t variant = n <= MSM_OWNED_MAX ? 2u : 0u;
    // The bucket reduction (see msm_task_reduce).  ONE bucket set with nothing else in flight on this context: by quads of lanes.  A batch of two is
    // 2048 waves of quads — two per SIMD, every step twice as long: 269 us inside a proof against ~230 lane-wise; the quads do the same additions in
    // 1.5x the lane-instructions, which a stream of commitments — whose reductions share the GPU with the next accumulation — pays for (three in flight
    // at 2^16 terms 0.243 -> 0.255 ms, measured); and above 2^20 terms a commitment has 3 or 5 bucket sets: 5120 tasks are five waves of quads per SIMD
    // (0.71 ms at 2^22 terms against ~0.45 lane-wise).
    // Otherwise lane-wise: 16 lanes per task for a batch of three or more commitments or when another commitment is in flight (a stream of commitments is
    // work-bound — every reduction wave displaces an accumulation wave of the next commitment for as long as it lives — and 16 lanes per task are fewer
    // wave-microseconds) and the addition built from lockstep product pairs (msm_task_reduce<.., true>: 19 % fewer instructions per addition; 8 lanes per task
    // were measured on top and lost, profiles/msm_nonloop_diet_ab.txt), 32 lanes and the latency-bound addition when latency is all that counts.
    const uint32_t lanes = (total_sets == 1 && !others_in_flight) ? 4u : ((batch >= 3 || others_in_flight) ? 16u : 32u);
    P.grid_reduce = (max_tasks * (lanes == 16 ? 16u : 32u) + MSM_THREADS - 1) / MSM_THREADS;
    P.grid_reduce_quad = (max_tasks + MSM_THREADS / 64 - 1) / (MSM_THREADS / 64);
    P.grid_bin_fold = (total_bins + MSM_THREADS / 64 - 1) / (MSM_THREADS / 64);
    P.roles = WS_FIRST_F_ROLE + (p.nbins + MSM_THREADS - 1) / MSM_THREADS - 1 + 1;
    P.bytes_pinned = (size_t)P.roles * total_sets * MSM_BYTES_XYZZ;
    plk_msm_shape &sh = P.shape;
    sh.path = PLK_MSM_PATH_ORDINARY;
    sh.table_copies = copies; sh.window_bits = p.c; sh.windows = p.windows; sh.bucket_sets = p.groups;
    sh.fine_bits = p.fine_bits; sh.coarse_bins = p.nbins;
    sh.accumulate_variant = variant; sh.prephase = prephase; sh.reduce_lanes = lanes;
    return P;
}

// One pass of the kernels: `terms` <= MSM_PASS_MAX_TERMS, 1 <= batch <= MSM_MAX_BATCH (msm_enqueue_batch refuses anything else before it plans).
// (table_valid, table_copies) is the resident table BEFORE the call: small_wanted is decided from it, and only then does the caller hand
// `table_request` to ensure_base_table — on every enqueue, zero terms and the naive path included.
inline MsmPlan msm_plan_pass(uint64_t terms, uint32_t batch, uint64_t srs_n, bool table_valid, uint32_t table_copies, bool others_in_flight,
                             bool fused_allowed) {
    const uint32_t nbits = msm_index_bits(terms);
    const uint32_t key_copies = table_copies_for(srs_n);
    // short commitments (msm_small.hip) need all 15 copies of the table: every commitment of >= 4096 terms builds them anyway; a shorter one
    // only asks for them when the key is small enough for that to be cheap or has them already
    const bool small_wanted = terms >= 1 && terms <= MSM_SMALL_MAX && key_copies == MAX_COPIES &&
                              (terms >= MSM_NAIVE_BELOW || srs_n <= MSM_SMALL_CHEAP_KEY || (table_valid && table_copies == MAX_COPIES));
    const uint32_t c_bits = small_wanted ? COPY_SHIFT : (terms >= MSM_NAIVE_BELOW ? pick_window_bits(terms, key_copies > 1) : 0);
    // the table is asked for 1 copy when the window is not 17 bits, otherwise for table_copies_for(srs_n); the copies the commitment addresses
    // are the largest divisor of 15 that fits the 24-bit (copy, index) field of an entry
    uint32_t copies = 1, request = 1;
    if (c_bits == COPY_SHIFT) {
        copies = request = key_copies;
        while (copies > 1 && (MAX_COPIES % copies != 0 || ((uint64_t)copies << nbits) > MSM_PASS_MAX_TERMS)) copies--;
    }
    const bool small = small_wanted && copies == MAX_COPIES;  // the short path only with all 15
    MsmPlan P;
    if (terms == 0) P = msm_plan_nothing(terms, batch, srs_n);
    else if (terms < MSM_NAIVE_BELOW && !small) P = msm_plan_naive(terms, batch, srs_n);
    else if (small) {
        // three short launches instead of the 2^20-shaped pipeline (msm_small.hip); p is what a re-run after an overflow keeps
        P = msm_plan_nothing(terms, batch, srs_n);
        P.run = MSM_RUN_SHORT;
        P.copies = copies;
        P.p = msm_params(terms, batch, srs_n, copies, c_bits, nbits);
        P.shape.path = PLK_MSM_PATH_SHORT; P.shape.table_copies = copies;
        P.bytes_pinned = (size_t)MSM_MAX_BATCH * SM_PLANES_HOST * MSM_BYTES_XYZZ + 16;
    } else P = msm_plan_pipeline(terms, batch, srs_n, copies, c_bits, nbits, others_in_flight, fused_allowed);
    P.table_request = request;
    return P;
}

// A bucket list of a short commitment overflowed (msm_small.hip): the same inputs again at the finish, by the naive kernel below 4096 terms
// and by the pipeline otherwise, with the enqueue-time copies, window bits and index bits.  `others_in_flight` is evaluated at the finish
// (after the FIFO has let this commitment go); the caller runs the accumulation with no_inf = false.
inline MsmPlan msm_plan_fallback(const MsmPlan &s, bool others_in_flight, bool fused_allowed) {
    MsmPlan P = s.terms < MSM_NAIVE_BELOW ? msm_plan_naive(s.terms, s.shape.batch, s.srs_n)
                                          : msm_plan_pipeline(s.terms, s.shape.batch, s.srs_n, s.copies, s.p.c, s.p.nbits, others_in_flight, fused_allowed);
    P.shape.path = PLK_MSM_PATH_SHORT_FALLBACK;               // with the re-run's fields
    P.shape.table_copies = P.copies = s.copies;
    return P;
}

// ---------------------------------------------------------------------------------------------- the plan of one call
// plk_msm_g1 / _dev / _partial_dev: long commitments as 2^20-term pieces, MSM_SLOTS in flight (see MSM_PIPELINE_MIN_TERMS) — only when the
// FIFO is empty at the call (it is, unless the caller keeps commitments in flight); otherwise passes of 2^24 terms, one at a time.
struct MsmCallPlan { uint64_t piece_terms, pieces; uint32_t depth; };
inline MsmCallPlan msm_plan_call(uint64_t terms, uint64_t srs_n, bool fifo_empty) {
    const bool pipelined = terms >= MSM_PIPELINE_MIN_TERMS && table_copies_for(srs_n) > 1 && fifo_empty;
    MsmCallPlan C;
    C.piece_terms = pipelined ? MSM_PIPELINE_PIECE : MSM_PASS_MAX_TERMS;
    C.depth = pipelined ? MSM_SLOTS : 1;
    C.pieces = terms ? (terms + C.piece_terms - 1) / C.piece_terms : 1;
    return C;
}

// ---------------------------------------------------------------------------------------------- caller-supplied bases
// plk_msm_g1_bases / _dev / _batch_dev: the points are the caller's, converted once per pass into a scratch of `terms` records — no key, so no
// table: ONE copy, the window widths of a key without shifted copies (13 / 15 / 17 bits), one bucket set per window, the pre-phase through
// the digit array.  Never the short path (it needs all 15 copies) and never another commitment in flight (the calls refuse that).
inline MsmPlan msm_plan_bases_pass(uint64_t terms, uint32_t batch, bool fused_allowed) {
    MsmPlan P;
    if (terms == 0) P = msm_plan_nothing(terms, batch, terms);
    else if (terms < MSM_NAIVE_BELOW) P = msm_plan_naive(terms, batch, terms);
    else P = msm_plan_pipeline(terms, batch, /*srs_n*/ terms, /*copies*/ 1, pick_window_bits(terms, false), msm_index_bits(terms),
                               /*others_in_flight*/ false, fused_allowed);
    P.table_request = 0;
    return P;
}
// one call: passes of 2^24 terms, one at a time, partial sums added on the host
inline MsmCallPlan msm_plan_bases_call(uint64_t terms) {
    MsmCallPlan C;
    C.piece_terms = MSM_PASS_MAX_TERMS;
    C.depth = 1;
    C.pieces = terms ? (terms + C.piece_terms - 1) / C.piece_terms : 1;
    return C;
}

}  // namespace plk
