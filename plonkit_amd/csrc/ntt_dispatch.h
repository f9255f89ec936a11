// Which passes a scalar transform is given: every dispatch decision of the NTT driver (ntt.hip, and the batching rule of prover.hip) and every
// constant it rests on, as pure functions of integers.  Host code only: no HIP include, no environment, no context, no allocation — so a
// stand-alone program checks the whole dispatch in seconds (tests/host/ntt_dispatch_check.cpp, tests/test_ntt_dispatch_host.py).
//   ntt_plan               one call of the driver (ntt_run): digits, tile, and per pass the kernel (role, family, template row bits and tile),
//                          the geometry NttPassArgs carries, the scalings, where it reads and writes, grid, block, LDS bytes, and the
//                          inter-pass twiddle table it wants
//   ntt_plan_has_scale     the one decision that waits for a runtime fact: 1/n on the last pass unless the first table took it
//   ntt_coset_direct_wanted  whether lde4cm_batch_dev / icoset4cm_dev keep their coset powers as per-element tables
//   ntt_batch_per_launch   transforms per launch of the four callers that split a batch
//   ntt_plan_eviction      which resident twiddle tables go when a new one does not fit under the cap
// ntt.hip's host side computes a plan, then reserves, obtains tables, fills NttPassArgs and launches; it decides nothing.  (ntt_plan.h is the
// index plan INSIDE a wave-owned tile; this header is the plan of the launches.)
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "ntt_plan.h"

namespace plk {

// ---------------------------------------------------------------------------------------------- constants
constexpr uint32_t MAX_LOG_N = 28;          // 2-adicity of Fr
constexpr uint32_t POW_SPLIT = 14;          // two-level power tables: e = hi * 2^14 + lo
constexpr uint32_t POW_TAB = 1u << POW_SPLIT;

constexpr int NTT_THREADS = 512;               // 8 waves per workgroup, 2 workgroups per CU (LDS): 4 waves per SIMD
constexpr int LOG_TILE = NTT_LOG_TILE;         // 2048 elements per workgroup
constexpr int LOG_SINGLE = 11;                 // largest transform done by one workgroup in one pass (ntt_pass_rows)
constexpr uint32_t NTT_MAX_BATCH = 16;         // transforms of equal shape sharing one launch per pass (blockIdx.y)
constexpr size_t NTT_BYTES_FR = 32, NTT_BYTES_SLOT = 36;     // an element in HBM, and in LDS (9 x 29-bit limbs)

// 11-bit digits on the 4096-element tile: 2^21 = 11 + 10 in two passes instead of three (0.207 -> 0.194 ms, same box).  2^22 = 11 + 11 is NOT
// taken: both passes then run on 64-byte row segments (C = 2) and the transform is 12 % SLOWER than three passes of the 2048-element tile
// (0.375 -> 0.421 ms; profiles/r06_ntt_big_tile_ab.txt)
constexpr uint32_t NTT_BIG_TILE_LOG_N = 21;

// dynamic LDS the kernels are allowed (hipFuncAttributeMaxDynamicSharedMemorySize, set once per process): every pass of a family asks for at
// most its family's size — the wave-owned kernels for exactly it
constexpr size_t NTT_LDS_ROWS = NTT_BYTES_SLOT << LOG_SINGLE;               // ntt_pass_rows: a whole transform of up to 2^11 points
constexpr size_t NTT_LDS_COLS = 96 * 1024;                                  // ntt_pass_cols
constexpr size_t NTT_W_LDS = NTT_BYTES_SLOT * NTT_W_SLOTS;                  // ntt_pass_w<7..10, *>
constexpr size_t NTT_W_LDS_BIG = NTT_BYTES_SLOT * NTT_W_SLOTS_BIG;          // ntt_pass_w<11, false, 12>, <10, true, 12>

// inter-pass twiddle tables (ntt_direct_table): a pass over a sub-transform of more than 2^POW_SPLIT points (below that its twiddles come straight
// out of the hi table) and of at most 2^25 (1 GiB per table); requests for the last NTT_DIRECT_KEEP tables asked for are never evicted
constexpr uint32_t NTT_DIRECT_MAX_LOG = 25;
constexpr uint64_t NTT_DIRECT_KEEP = 96;
constexpr size_t NTT_DIRECT_CAP_DEFAULT_MB = 6144;
// per-element coset tables of the extensions (coset_direct_tables): POW_SPLIT < log_n <= 24 (4 x n entries: 2 GiB at 2^24)
constexpr uint32_t NTT_COSET_DIRECT_MAX_LOG = 24;
// callers that split a batch keep the ping-pong scratch of one launch at 2 GiB where more than one transform shares it
constexpr size_t NTT_BATCH_SCRATCH_MAX = (size_t)2 << 30;
// the prover's own batches (wire, selector and sigma columns): four per launch up to this domain, one at a time above
constexpr uint32_t NTT_PROVER_BATCH_MAX_LOG = 22, NTT_PROVER_BATCH = 4;

// ---------------------------------------------------------------------------------------------- the plan of one transform call
enum : uint32_t { NTT_SCALE_NONE = 0,       // no coset shift on this side
                  NTT_SCALE_TWO_LEVEL = 1,  // powers composed from a two-level table (PowTable): two loads and a product per element
                  NTT_SCALE_PER_ELEMENT = 2 };   // powers read from a table of their own (beside the two-level one, which the kernels ignore then)
enum : uint32_t { NTT_ROLE_COLS = 0,        // passes 1..p-1: digit i of every column, rows fetched bit-reversed, inter-pass twiddles on store
                  NTT_ROLE_ROWS = 1 };      // the last pass: contiguous rows, digit-reversed output index, output scaling and 1/n
enum : uint32_t { NTT_FAMILY_BARRIER = 0,   // ntt_pass_cols / ntt_pass_rows: any tile of up to 2^11 elements, 512 threads
                  NTT_FAMILY_WAVE = 1 };    // ntt_pass_w<row_bits, role, log_tile>: full tiles only
enum : uint32_t { NTT_AT_SOURCE = 0, NTT_AT_SCRATCH = 1, NTT_AT_DATA = 2 };

constexpr uint32_t NTT_MAX_PASSES = 3;

struct NttPassPlan {
    uint32_t role, family;
    uint32_t row_bits, log_tile;                // the template arguments of a wave pass (0, 0 for a barrier pass)
    uint32_t log_r, log_c, log_inner;           // NttPassArgs, as the kernels read them
    uint32_t log_r1, log_m1, log_m2;
    uint32_t nonzero;
    uint32_t quarter;                           // see ntt_plan_passes: one shape only
    uint32_t pre, post;                         // NTT_SCALE_*: input scaling (first pass), output scaling (last pass)
    uint32_t reads, writes;                     // NTT_AT_*
    uint32_t grid_x, block, lds_bytes;          // grid.y is the plan's count
    uint32_t wants_table;                       // inter-pass twiddles as a table of 2^table_bits entries under table_key,
    uint32_t table_bits, table_key;             //   if the cap and the device memory allow it (otherwise the pass composes them)
    uint32_t table_scaled;                      // 1/n folded into that table (first pass of an inverse transform)
};

// (64-bit member first, an even number of 32-bit ones: no padding, so equal plans are equal bytes)
struct NttPlan {
    size_t scratch_bytes;                       // ping-pong buffer: count x n elements when there is more than one pass
    uint32_t log_n, count, inverse;
    uint32_t passes, log_tile;                 // log_tile: 11, or 12 for the 11 + 10 plan
    uint32_t digit[4];                          // digit[i]: the bits pass i transforms; zero beyond `passes`
    NttPassPlan pass[NTT_MAX_PASSES];
};
static_assert(sizeof(NttPassPlan) == 23 * 4 && sizeof(NttPlan) == sizeof(size_t) + 9 * 4 + NTT_MAX_PASSES * sizeof(NttPassPlan), "NttPlan has padding");

// Digits of the mixed-radix plan on the 2048-element tile: one pass — ONE workgroup holds the whole transform in LDS — up to 2^11 points (2^12
// points in one workgroup, 147 KB of the CU's 160 KB, was tried and is SLOWER than two passes of two workgroups: 62 against 37 us per transform,
// same box); otherwise up to 10 bits per pass, split evenly: 2^20 = 10 + 10.
inline uint32_t ntt_digits(uint32_t log_n, uint32_t d[4]) {
    d[0] = d[1] = d[2] = d[3] = 0;
    if (log_n <= (uint32_t)LOG_SINGLE) { d[0] = log_n; return 1; }
    const uint32_t p = (log_n + 9) / 10;
    for (uint32_t i = 0; i < p; i++) d[i] = log_n / p + (i < log_n % p ? 1 : 0);
    if (p == 3 && log_n <= 23) {                           // leave 14 bits to passes 2 and 3: their inter-pass twiddles
        d[0] = log_n - 14; d[1] = 7; d[2] = 7;             // then come straight out of the hi table (ntt_pass_cols)
    }
    return p;
}

// key of an inter-pass table: injective over (direction, the log_n whose 1/n is folded in or 0, log_r, log_inner), all below 2^5 but the first
inline uint32_t ntt_table_key(bool inverse, uint32_t folded_log_n, uint32_t log_r, uint32_t log_inner) {
    return (inverse ? 1u << 31 : 0) | folded_log_n << 16 | log_r << 8 | log_inner;
}

// The passes for given digits and tile.  The family of a pass follows from its own shape here and nowhere else: wave-owned when the tile is
// full (log_r + log_c = log_tile) with row bits TilePlan accepts — 7..10 on the 2048-element tile, the 11 + 10 plan on the 4096-element one —
// and the pass does not have to skip a zero-padded tail while reading a per-element input table (the wave kernels take zero-padded inputs,
// and per-element tables, but were never given both); a single pass is always the barrier kernel.
inline NttPlan ntt_plan_passes(uint32_t log_n, uint32_t count, bool inverse, uint64_t nonzero, uint32_t pre, uint32_t post, bool tables_allowed,
                               const uint32_t d[4], uint32_t p, uint32_t log_tile) {
    NttPlan P{};
    P.log_n = log_n; P.count = count; P.inverse = inverse ? 1u : 0u; P.passes = p; P.log_tile = log_tile;
    for (uint32_t i = 0; i < 4; i++) P.digit[i] = d[i];
    const size_t n = (size_t)1 << log_n;
    P.scratch_bytes = p > 1 ? (size_t)count * n * NTT_BYTES_FR : 0;
    uint32_t rem = log_n;
    for (uint32_t i = 0; i < p; i++) {
        NttPassPlan &q = P.pass[i];
        const bool first = i == 0, last = i + 1 == p;
        rem -= d[i];
        q.role = last ? NTT_ROLE_ROWS : NTT_ROLE_COLS;
        q.log_r = d[i];
        if (!last) {
            q.log_inner = rem;
            q.log_c = (log_tile - d[i]) < rem ? (log_tile - d[i]) : rem;
        } else if (p > 1) {
            q.log_r1 = d[0];
            q.log_m1 = p >= 3 ? d[1] : 0;                  // (log_m2 stays 0: no plan has a fourth digit)
            q.log_c = (log_tile - d[i]) < d[0] ? (log_tile - d[i]) : d[0];
        }
        // ping-pong: pass 1 source -> scratch, middle passes in place in scratch, last pass scratch -> data.  (A single pass is one workgroup per
        // transform that has read ALL of its input into LDS — a barrier — before its first store: in place is safe, no detour through the scratch)
        q.reads = first ? NTT_AT_SOURCE : NTT_AT_SCRATCH;
        q.writes = last ? NTT_AT_DATA : NTT_AT_SCRATCH;
        q.nonzero = first ? (uint32_t)nonzero : 0;
        q.pre = first ? pre : NTT_SCALE_NONE;
        q.post = last ? post : NTT_SCALE_NONE;
        const uint32_t tile = q.log_r + q.log_c;
        const bool full = tile == log_tile && (log_tile == (uint32_t)NTT_LOG_TILE_BIG || (q.log_r >= 7 && q.log_r <= 10));
        q.family = (p > 1 && full && !(q.nonzero && q.pre == NTT_SCALE_PER_ELEMENT)) ? NTT_FAMILY_WAVE : NTT_FAMILY_BARRIER;
        q.grid_x = (uint32_t)(n >> tile);
        if (q.family == NTT_FAMILY_WAVE) {
            q.row_bits = q.log_r; q.log_tile = log_tile;
            q.block = log_tile == (uint32_t)NTT_LOG_TILE_BIG ? 2 * NTT_THREADS : NTT_THREADS;      // sixteen waves own the 4096-element tile
            q.lds_bytes = (uint32_t)(log_tile == (uint32_t)NTT_LOG_TILE_BIG ? NTT_W_LDS_BIG : NTT_W_LDS);
        } else {
            q.block = NTT_THREADS;
            q.lds_bytes = (uint32_t)(NTT_BYTES_SLOT << tile);
        }
        // `quarter`: the barrier kernel's shortcut for the first pass of an extension by 4 with an even number of stages (only every fourth
        // bit-reversed row is non-zero, the first pair of stages is a broadcast).  One shape uses it: 4n = 2^12, the 6 + 6 plan — every other
        // size has an odd first digit (2^13) or a first pass the wave kernel takes, which has no such shortcut.
        q.quarter = (first && !last && q.family == NTT_FAMILY_BARRIER && nonzero && nonzero == (n >> 2) && !(d[0] & 1) && d[0] >= 2) ? 1 : 0;
        if (!last) {
            const uint32_t bits = q.log_r + q.log_inner;
            q.wants_table = (tables_allowed && bits > POW_SPLIT && bits <= NTT_DIRECT_MAX_LOG) ? 1 : 0;
            if (q.wants_table) {
                q.table_bits = bits;
                q.table_scaled = (inverse && first) ? 1 : 0;
                q.table_key = ntt_table_key(inverse, q.table_scaled ? log_n : 0, q.log_r, q.log_inner);
            }
        }
    }
    return P;
}

// One call of ntt_run: `count` transforms of 2^log_n points (1 <= log_n <= MAX_LOG_N, 1 <= count <= NTT_MAX_BATCH: the driver refuses anything
// else before it plans).  nonzero: input elements from this index on are zero (0 = the whole vector); pre / post: NTT_SCALE_* of the input and
// the output; tables_allowed: the caller's reading of PLK_NTT_DIRECT.
// The 4096-element tile is taken only where BOTH of its passes come out wave-owned: the barrier kernels cannot hold it (36 * 2^12 bytes of
// LDS against NTT_LDS_COLS, 512 threads, at most 2^11 elements).  Otherwise 2^21 is 7 + 7 + 7 on the 2048-element tile, like its neighbours.
inline NttPlan ntt_plan(uint32_t log_n, uint32_t count, bool inverse, uint64_t nonzero, uint32_t pre, uint32_t post, bool tables_allowed) {
    uint32_t d[4];
    if (log_n == NTT_BIG_TILE_LOG_N) {
        d[0] = 11; d[1] = 10; d[2] = d[3] = 0;
        const NttPlan P = ntt_plan_passes(log_n, count, inverse, nonzero, pre, post, tables_allowed, d, 2, (uint32_t)NTT_LOG_TILE_BIG);
        if (P.pass[0].family == NTT_FAMILY_WAVE && P.pass[1].family == NTT_FAMILY_WAVE) return P;
    }
    const uint32_t p = ntt_digits(log_n, d);
    return ntt_plan_passes(log_n, count, inverse, nonzero, pre, post, tables_allowed, d, p, (uint32_t)LOG_TILE);
}

// 1/n on the last pass of an inverse transform — unless the first pass's table, which has it folded in, was actually obtained (it is not when
// the cap or the device memory refuses it: a runtime fact the driver reports here)
inline uint32_t ntt_plan_has_scale(const NttPlan &P, bool first_table_obtained) {
    return (P.inverse && !(P.pass[0].table_scaled && first_table_obtained)) ? 1u : 0u;
}

// the coset powers of lde4cm_batch_dev / icoset4cm_dev as per-element tables (up to 2^14 points the low table alone holds the power)
inline bool ntt_coset_direct_wanted(uint32_t log_n, bool tables_allowed) {
    return tables_allowed && log_n > POW_SPLIT && log_n <= NTT_COSET_DIRECT_MAX_LOG;
}

// ---------------------------------------------------------------------------------------------- the batch plan
enum : uint32_t { NTT_BATCH_PLAIN = 0,      // ntt_batch_dev: transforms of 2^log_n points
                  NTT_BATCH_LDE4 = 1,       // lde4_batch_dev: polynomials of 2^log_n coefficients, one 4n-point transform each
                  NTT_BATCH_LDE4CM = 2,     // lde4cm_batch_dev: polynomials of 2^log_n coefficients, FOUR n-point transforms each
                  NTT_BATCH_PROVER = 3 };   // the prover's column batches: transforms of 2^log_n points
// Items (transforms; polynomials for the two extensions) that share one launch per pass.  Never more than NTT_MAX_BATCH transforms, and no more
// than NTT_BATCH_SCRATCH_MAX of ping-pong scratch unless a single item needs it.
inline uint32_t ntt_batch_per_launch(uint32_t rule, uint32_t log_n) {
    uint32_t per;
    switch (rule) {
        case NTT_BATCH_LDE4:                               // 16 / 4 / 1: up to 4n = 2^22 / 2^24 / beyond
            for (per = NTT_MAX_BATCH; per > 1 && ((size_t)per * NTT_BYTES_FR << (log_n + 2)) > NTT_BATCH_SCRATCH_MAX;) per /= 4;
            return per;
        case NTT_BATCH_LDE4CM:
            for (per = NTT_MAX_BATCH / 4; per > 1 && ((size_t)per * 4 * NTT_BYTES_FR << log_n) > NTT_BATCH_SCRATCH_MAX;) per--;
            return per;
        case NTT_BATCH_PROVER:
            return log_n <= NTT_PROVER_BATCH_MAX_LOG ? NTT_PROVER_BATCH : 1;
        default:
            return NTT_MAX_BATCH;
    }
}

// ---------------------------------------------------------------------------------------------- eviction of inter-pass twiddle tables
// A long-lived context that proves many domain sizes would otherwise collect tables for ever (up to 1 GiB each).  When the next one would take
// the total past the cap, the tables that have not been asked for during the last NTT_DIRECT_KEEP requests (about two proofs' worth) go, oldest
// first, and only as many as it takes.  Tables of the plan in use are never dropped: if they alone fill the cap (a small PLK_NTT_DIRECT_CAP_MB,
// or one proof whose shapes exceed it) the new pass composes its twiddles instead — dropping everything made such a proof rebuild its tables,
// and stall every stream, on every pass.
struct NttResident { uint32_t key; uint64_t used; size_t bytes; };     // a resident table: `used` = the clock at its last request
constexpr int NTT_EVICT_COMPOSE = -1;
// Returns how many keys it wrote to drop[] (room for `count`), in the order they go, or NTT_EVICT_COMPOSE.  `clock` is the number of this request.
inline int ntt_plan_eviction(const NttResident *res, size_t count, uint64_t clock, size_t want, size_t cap, uint32_t *drop) {
    size_t held = 0;
    for (size_t i = 0; i < count; i++) held += res[i].bytes;
    int dropped = 0;
    uint64_t after_used = 0; uint32_t after_key = 0; bool any = false;      // the last table chosen: the next one is the smallest (used, key) above it
    while (held + want > cap) {
        size_t best = count;
        for (size_t i = 0; i < count; i++) {
            const NttResident &r = res[i];
            if (!(r.used + NTT_DIRECT_KEEP < clock)) continue;                                    // asked for recently
            if (any && (r.used < after_used || (r.used == after_used && r.key <= after_key))) continue;      // gone already
            if (best == count || r.used < res[best].used || (r.used == res[best].used && r.key < res[best].key)) best = i;
        }
        if (best == count) return NTT_EVICT_COMPOSE;                  // the tables in use fill the cap
        after_used = res[best].used; after_key = res[best].key; any = true;
        held -= res[best].bytes;
        drop[dropped++] = res[best].key;
    }
    return dropped;
}

}  // namespace plk
