// Stand-alone check of plonkit_amd/csrc/msm_plan.h (which kernels a commitment is given).  Built with -fsanitize=address,undefined by
// tests/test_msm_plan_host.py and run directly.  Every decision comes from the header's functions; this program only keeps the books the
// library keeps around them: the FIFO of commitments in flight and the resident table of a key.
//   msm_plan_check table   reads one line per row of tests/test_gpu_msm_shapes.py from stdin ("key srs_n terms batch style overflow"), key by key
//                          in table order, and prints the thirteen fields of plk_msm_shape the row ends with
//   msm_plan_check sweep   invariants of the plan over a grid of (terms, batch, key size, table state, in flight, fused allowed)
#include "../../plonkit_amd/csrc/msm_plan.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

using namespace plk;

// ensure_base_table (msm.hip): the table is rebuilt with the requested copies unless it is valid with at least as many
struct Table { bool valid = false; uint32_t copies = 0; };
static void ensure(Table &t, uint32_t request) {
    if (t.valid && t.copies >= request) return;
    t.valid = true; t.copies = request;
}

static const char *PATHS[5] = {"empty", "naive", "short", "short_fallback", "ordinary"};     // PLK_MSM_PATH_*

static int table_mode() {
    std::map<std::string, Table> tables;                      // every key starts without a table
    char key[64], style[64];
    unsigned long long srs_n, terms;
    unsigned batch, overflow;
    int rows = 0;
    while (scanf("%63s %llu %llu %u %63s %u", key, &srs_n, &terms, &batch, style, &overflow) == 6) {
        Table &t = tables[key];
        MsmPlan P;
        MsmCallPlan call{terms, 1, 1};
        if (!strcmp(style, "inflight")) {                      // one other commitment of the same length is enqueued first and finished first
            P = msm_plan_pass(terms, 1, srs_n, t.valid, t.copies, false, true);
            ensure(t, P.table_request);
            P = msm_plan_pass(terms, 1, srs_n, t.valid, t.copies, true, true);
            ensure(t, P.table_request);
        } else if (batch == 1) {                               // plk_msm_g1_dev: the FIFO is empty at the call; its loop of plk_msm_g1_partial_dev
            call = msm_plan_call(terms, srs_n, true);
            uint64_t off = 0;
            uint32_t inflight = 0;
            if (call.pieces == 1) {                            // one pass
                P = msm_plan_pass(terms, 1, srs_n, t.valid, t.copies, false, true);
                ensure(t, P.table_request);
            } else do {                                        // "others in flight" = pieces enqueued and not finished
                while (off < terms && inflight < call.depth) {
                    const uint64_t len = terms - off < call.piece_terms ? terms - off : call.piece_terms;
                    P = msm_plan_pass(len, 1, srs_n, t.valid, t.copies, inflight != 0, true);
                    ensure(t, P.table_request);
                    off += call.piece_terms; inflight++;
                }
                inflight--;                                    // the oldest piece is finished
            } while (off < terms || inflight);
        } else {                                               // plk_msm_g1_batch_dev: one batch, nothing else in flight
            P = msm_plan_pass(terms, batch, srs_n, t.valid, t.copies, false, true);
            ensure(t, P.table_request);
        }
        if (overflow) {                                        // a bucket list overflows: the re-run at the finish, alone on the context by then
            if (P.run != MSM_RUN_SHORT) { fprintf(stderr, "row %d: an overflow row that is not on the short path\n", rows); return 1; }
            P = msm_plan_fallback(P, false, true);
        }
        plk_msm_shape s = P.shape;
        if (call.pieces > 1) { s.pieces = (uint32_t)call.pieces; s.piece_terms = call.piece_terms; }    // (plk_msm_last_shape: the multi-piece path only)
        if (s.path > 4) { fprintf(stderr, "row %d: path %u\n", rows, s.path); return 1; }
        printf("%s %u %u %u %u %u %u %u %u %u %u %u %llu\n", PATHS[s.path], s.batch, s.table_copies, s.window_bits, s.windows, s.bucket_sets, s.fine_bits,
               s.coarse_bins, s.accumulate_variant, s.prephase, s.reduce_lanes, s.pieces, (unsigned long long)s.piece_terms);
        rows++;
    }
    fprintf(stderr, "msm_plan_check: %d rows\n", rows);
    return 0;
}

static long failures = 0, cases = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures++ < 40) { fprintf(stderr, "FAIL %s:%d: %s — ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)
#define FITS32(value64, value32) ((uint64_t)(value64) == (uint64_t)(value32) && (uint64_t)(value64) <= 0xffffffffull)

static void check_pipeline(const MsmPlan &P, uint64_t n, uint32_t batch, uint64_t srs_n, bool others, bool fused, const char *what) {
    const MsmParams &p = P.p;
    const uint32_t c = p.c, copies = P.copies;
    EXPECT(c == 13 || c == 15 || c == 17, "%s: window bits %u", what, c);
    EXPECT(p.windows == 254 / c + 1 && P.shape.windows == p.windows && P.shape.window_bits == c, "%s: windows %u for c = %u", what, p.windows, c);
    EXPECT(p.fine_bits == FINE_BITS && p.coarse_bits == c - 1 - FINE_BITS && p.nbins == 1u << (c - 1 - FINE_BITS) && p.nbins <= 1024 && P.shape.coarse_bins == p.nbins,
           "%s: %u coarse bins for c = %u", what, p.nbins, c);
    EXPECT(p.n == n && p.batch == batch && p.nbits == msm_index_bits(n), "%s: n, batch, nbits", what);
    if (copies > 1) EXPECT(c == COPY_SHIFT && p.groups * copies == p.windows, "%s: %u bucket sets x %u copies != %u windows", what, p.groups, copies, p.windows);
    else EXPECT(p.groups == p.windows, "%s: one copy, %u bucket sets, %u windows", what, p.groups, p.windows);
    EXPECT(P.shape.bucket_sets == p.groups && P.shape.table_copies == copies, "%s: reported sets / copies", what);
    // 64-bit restatement of every 32-bit product
    const uint64_t stride = copies > 1 ? (uint64_t)p.groups * srs_n : 0;
    EXPECT(FITS32(stride, p.copy_stride), "%s: copy_stride %llu", what, (unsigned long long)stride);
    const uint64_t total_sets = (uint64_t)batch * p.groups, total_bins = total_sets * p.nbins, total_windows = (uint64_t)batch * p.windows;
    const uint64_t max_tasks = total_bins + total_windows * n / TASK_MAX + 1;
    EXPECT(FITS32(total_sets, P.total_sets) && FITS32(total_bins, P.total_bins) && FITS32(total_windows, P.total_windows) && FITS32(max_tasks, P.max_tasks),
           "%s: totals (%llu sets, %llu bins, %llu windows, %llu tasks)", what, (unsigned long long)total_sets, (unsigned long long)total_bins,
           (unsigned long long)total_windows, (unsigned long long)max_tasks);
    // the decisions
    const uint32_t prephase = (fused && p.groups == 1 && c == 17) ? 1 : 2;
    const uint32_t lanes = (total_sets == 1 && !others) ? 4 : ((batch >= 3 || others) ? 16 : 32);
    EXPECT(P.shape.prephase == prephase, "%s: pre-phase %u", what, P.shape.prephase);
    EXPECT(P.shape.accumulate_variant == (n <= (1ull << 16) ? 2u : 0u), "%s: variant %u", what, P.shape.accumulate_variant);
    EXPECT(P.shape.reduce_lanes == lanes, "%s: %u reduction lanes", what, P.shape.reduce_lanes);
    const uint64_t roles = 9 + (p.nbins + 255) / 256;
    EXPECT(P.roles == roles && roles <= 13, "%s: %u roles", what, P.roles);
    // grids
    if (prephase == 1) {
        EXPECT(FITS32((n + 4095) / 4096, P.grid_recode_count) && FITS32((n + 1023) / 1024, P.grid_recode_scatter) && P.grid_digits == 0 && P.grid_partition == 0,
               "%s: fused grids", what);
        EXPECT(P.lds_recode_scatter == (3 * (size_t)p.nbins + 1 + 1024 * 15) * 4 && P.lds_recode_scatter <= 96 * 1024, "%s: fused LDS", what);
    } else {
        EXPECT(FITS32((n + 255) / 256, P.grid_digits) && FITS32((n + DIGIT_CHUNK - 1) / DIGIT_CHUNK, P.grid_partition) && P.grid_recode_count == 0 && P.grid_recode_scatter == 0,
               "%s: digit-array grids", what);
        EXPECT(P.lds_partition_count == (size_t)p.nbins * 4 && P.lds_partition_scatter == (3 * (size_t)p.nbins + 1 + DIGIT_CHUNK) * 4 && P.lds_partition_scatter <= 96 * 1024,
               "%s: partition LDS", what);
        EXPECT(total_windows <= 65535, "%s: %llu windows in gridDim.y", what, (unsigned long long)total_windows);
    }
    EXPECT(FITS32((max_tasks * (lanes == 16 ? 16 : 32) + 255) / 256, P.grid_reduce) && FITS32((max_tasks + 3) / 4, P.grid_reduce_quad) && FITS32((total_bins + 3) / 4, P.grid_bin_fold),
           "%s: reduction grids", what);
    EXPECT(P.grid_naive == 0, "%s: naive grid on the pipeline", what);
    // the buffers, as msm_big_launch sized them before the plan existed (XyzzW 144 B, G1Xyzz 128 B, Fr 32 B)
    EXPECT(P.bytes_a == (size_t)(3 * total_bins + 4) * 4, "%s: a", what);
    EXPECT(P.bytes_b == (size_t)(total_windows * n * 4), "%s: b", what);
    EXPECT(P.bytes_c == (size_t)(max_tasks * 2 * 144 + max_tasks * ((1u << FINE_BITS) + 2) * 4), "%s: c", what);
    EXPECT(P.bytes_d == (size_t)(13 * total_sets * 128), "%s: d", what);
    EXPECT(P.bytes_e == (size_t)(max_tasks * ((1u << FINE_BITS) + 2 * 256) * 144), "%s: e", what);
    EXPECT(P.bytes_f == (size_t)(prephase == 1 ? batch * n * 32 : total_windows * n * 4), "%s: f", what);
    EXPECT(P.bytes_pinned == (size_t)(roles * total_sets * 128) && P.bytes_pinned <= P.bytes_d, "%s: pinned", what);
}

static void check_naive(const MsmPlan &P, uint64_t n, uint32_t batch, const char *what) {
    EXPECT(n >= 1 && n < 4096, "%s: naive with %llu terms", what, (unsigned long long)n);
    EXPECT(FITS32((n + 255) / 256, P.grid_naive) && P.bytes_d == (size_t)batch * P.grid_naive * 128 && P.bytes_pinned == P.bytes_d, "%s: naive grid and buffers", what);
    EXPECT(P.shape.window_bits == 0 && P.shape.windows == 0 && P.shape.bucket_sets == 0 && P.shape.reduce_lanes == 0 && P.shape.prephase == 0, "%s: naive reports a pipeline", what);
}

static int sweep_mode() {
    const uint64_t P15 = 1ull << 15, P16 = 1ull << 16, P17 = 1ull << 17, P19 = 1ull << 19, P20 = 1ull << 20, P21 = 1ull << 21, P22 = 1ull << 22, P24 = 1ull << 24;
    const uint64_t TERMS[] = {0, 1, 4095, 4096, 4097, P15, P15 + 1, P16, P16 + 1, P17 - 1, P17, P19 - 1, P19, P20, P20 + 1, P21, P21 + 1, P22, P22 + 1, P24};
    const uint64_t KEYS[] = {P16, P21, P21 + 1, 35791394, 35791395, 1ull << 26};
    const Table STATES[] = {{false, 0}, {true, 1}, {true, 15}};
    for (uint64_t n : TERMS) for (uint32_t batch = 1; batch <= 8; batch++) for (uint64_t srs_n : KEYS) {
        if (n > srs_n) continue;
        for (const Table &t : STATES) for (int others = 0; others < 2; others++) for (int fused = 0; fused < 2; fused++) {
            cases++;
            char what[160];
            snprintf(what, sizeof what, "n=%llu batch=%u srs_n=%llu table=%d/%u others=%d fused=%d", (unsigned long long)n, batch, (unsigned long long)srs_n,
                     (int)t.valid, t.copies, others, fused);
            const MsmPlan P = msm_plan_pass(n, batch, srs_n, t.valid, t.copies, others != 0, fused != 0);
            const MsmPlan Q = msm_plan_pass(n, batch, srs_n, t.valid, t.copies, others != 0, fused != 0);
            EXPECT(memcmp(&P, &Q, sizeof P) == 0, "%s: two plans of the same inputs differ", what);
            const uint32_t key_copies = table_copies_for(srs_n);
            EXPECT(key_copies == (srs_n <= 35791394 ? 15u : 1u), "%s: table_copies_for", what);
            EXPECT(P.table_request == 1 || P.table_request == key_copies, "%s: asks the table for %u copies", what, P.table_request);
            EXPECT(P.copies >= 1 && 15 % P.copies == 0 && ((uint64_t)P.copies << P.p.nbits) <= P24 && P.copies <= P.table_request, "%s: addresses %u copies, nbits %u", what, P.copies, P.p.nbits);
            EXPECT((1ull << P.p.nbits) >= n && P.p.nbits >= 1 && (P.p.nbits == 1 || (1ull << (P.p.nbits - 1)) < n), "%s: nbits %u", what, P.p.nbits);
            EXPECT(P.terms == n && P.srs_n == srs_n && P.shape.batch == batch && P.shape.pieces == 1 && P.shape.piece_terms == n, "%s: the record of the inputs", what);
            switch (P.run) {
            case MSM_RUN_NOTHING:
                EXPECT(n == 0 && P.shape.path == PLK_MSM_PATH_EMPTY && P.shape.table_copies == 0 && P.bytes_pinned == 0, "%s: nothing to run", what);
                break;
            case MSM_RUN_NAIVE:
                EXPECT(P.shape.path == PLK_MSM_PATH_NAIVE && P.shape.table_copies == 1 && P.table_request == 1, "%s: naive", what);
                check_naive(P, n, batch, what);
                break;
            case MSM_RUN_SHORT: {
                EXPECT(P.shape.path == PLK_MSM_PATH_SHORT && P.copies == 15 && P.shape.table_copies == 15 && P.table_request == 15 && n >= 1 && n <= P15, "%s: short", what);
                EXPECT(n >= 4096 || srs_n <= P21 || (t.valid && t.copies == 15), "%s: short path below 4096 terms on a large key without its table", what);
                EXPECT(P.p.c == 17 && FITS32(srs_n, P.p.copy_stride) && P.bytes_pinned == 8 * 17 * 128 + 16, "%s: short launch parameters", what);
                for (int late = 0; late < 2; late++) {         // the re-run after an overflow keeps copies, c and nbits; naive below 4096 terms
                    const MsmPlan F = msm_plan_fallback(P, late != 0, fused != 0);
                    EXPECT(F.shape.path == PLK_MSM_PATH_SHORT_FALLBACK && F.copies == 15 && F.shape.table_copies == 15 && F.shape.batch == batch && F.shape.piece_terms == n, "%s: fallback", what);
                    EXPECT(F.run == (n < 4096 ? (uint32_t)MSM_RUN_NAIVE : (uint32_t)MSM_RUN_PIPELINE), "%s: fallback runs %u", what, F.run);
                    if (F.run == MSM_RUN_NAIVE) check_naive(F, n, batch, what);
                    else { EXPECT(F.p.c == 17 && F.p.nbits == P.p.nbits, "%s: fallback c / nbits", what); check_pipeline(F, n, batch, srs_n, late != 0, fused != 0, what); }
                }
                break;
            }
            case MSM_RUN_PIPELINE: {
                EXPECT(P.shape.path == PLK_MSM_PATH_ORDINARY && n >= 4096 && (n > P15 || key_copies == 1), "%s: pipeline", what);
                EXPECT(P.p.c == (key_copies > 1 ? 17u : (n < P17 ? 13u : (n < P19 ? 15u : 17u))), "%s: c = %u", what, P.p.c);
                EXPECT(P.table_request == (P.p.c == 17 ? key_copies : 1u), "%s: request %u at c = %u", what, P.table_request, P.p.c);
                check_pipeline(P, n, batch, srs_n, others != 0, fused != 0, what);
                const MsmPlan H = msm_plan_pipeline(n, batch, srs_n, P.copies, P.p.c, P.p.nbits, others != 0, fused != 0);   // the half on its own
                MsmPlan H2 = H; H2.table_request = P.table_request;
                EXPECT(memcmp(&H2, &P, sizeof P) == 0, "%s: msm_plan_pipeline alone differs from the pass", what);
                break;
            }
            default: EXPECT(false, "%s: run %u", what, P.run);
            }
            if (n < 4096 && n >= 1) EXPECT(P.run == MSM_RUN_NAIVE || P.run == MSM_RUN_SHORT, "%s: fewer than 4096 terms on the pipeline", what);
        }
    }
    // the plan of one call
    const uint64_t CALLS[] = {0, 1, (1ull << 23) - 1, 1ull << 23, (1ull << 23) + 100, P24, P24 + 1, 1ull << 26};
    for (uint64_t srs_n : KEYS) for (uint64_t n : CALLS) for (int empty = 0; empty < 2; empty++) {
        cases++;
        const MsmCallPlan C = msm_plan_call(n, srs_n, empty != 0);
        const bool pipelined = n >= (1ull << 23) && table_copies_for(srs_n) > 1 && empty;
        EXPECT(C.piece_terms == (pipelined ? P20 : P24) && C.depth == (pipelined ? 3u : 1u) && C.depth <= MSM_SLOTS, "call n=%llu srs_n=%llu empty=%d: piece %llu depth %u",
               (unsigned long long)n, (unsigned long long)srs_n, empty, (unsigned long long)C.piece_terms, C.depth);
        EXPECT(C.pieces >= 1 && C.pieces * C.piece_terms >= n && (C.pieces - 1) * C.piece_terms < (n ? n : 1), "call n=%llu: %llu pieces", (unsigned long long)n, (unsigned long long)C.pieces);
    }
    if (failures) { fprintf(stderr, "msm_plan_check: %ld failures in %ld cases\n", failures, cases); return 1; }
    printf("msm_plan_check: ok, %ld cases\n", cases);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "table")) return table_mode();
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep_mode();
    fprintf(stderr, "usage: msm_plan_check table < rows | msm_plan_check sweep\n");
    return 2;
}
