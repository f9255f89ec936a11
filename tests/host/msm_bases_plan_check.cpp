// Stand-alone check of the plan of a commitment against caller-supplied bases (plonkit_amd/csrc/msm_plan.h: msm_plan_bases_pass,
// msm_plan_bases_call).  Built with -fsanitize=address,undefined by tests/test_msm_bases_plan_host.py and run directly.
//   msm_bases_plan_check table   reads "terms batch" lines from stdin and prints the thirteen fields of plk_msm_shape of the pass
//   msm_bases_plan_check sweep   invariants of the pass plan and of the call plan over a grid of (terms, batch, fused allowed)
#include "../../plonkit_amd/csrc/msm_plan.h"
#include <cstdio>
#include <cstring>

using namespace plk;

static const char *PATHS[5] = {"empty", "naive", "short", "short_fallback", "ordinary"};     // PLK_MSM_PATH_*

static int table_mode() {
    unsigned long long terms;
    unsigned batch;
    int rows = 0;
    while (scanf("%llu %u", &terms, &batch) == 2) {
        const MsmPlan P = msm_plan_bases_pass(terms, batch, true);
        const plk_msm_shape &s = P.shape;
        if (s.path > 4) { fprintf(stderr, "row %d: path %u\n", rows, s.path); return 1; }
        printf("%s %u %u %u %u %u %u %u %u %u %u %u %llu\n", PATHS[s.path], s.batch, s.table_copies, s.window_bits, s.windows, s.bucket_sets, s.fine_bits,
               s.coarse_bins, s.accumulate_variant, s.prephase, s.reduce_lanes, s.pieces, (unsigned long long)s.piece_terms);
        rows++;
    }
    fprintf(stderr, "msm_bases_plan_check: %d rows\n", rows);
    return 0;
}

static long failures = 0, cases = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures++ < 40) { fprintf(stderr, "FAIL %s:%d: %s — ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)
#define FITS32(value64, value32) ((uint64_t)(value64) == (uint64_t)(value32) && (uint64_t)(value64) <= 0xffffffffull)

static void check_pass(uint64_t n, uint32_t batch, bool fused) {
    cases++;
    const MsmPlan P = msm_plan_bases_pass(n, batch, fused), again = msm_plan_bases_pass(n, batch, fused);
    EXPECT(!memcmp(&P, &again, sizeof P), "n = %llu batch %u: two plans of the same arguments differ", (unsigned long long)n, batch);
    EXPECT(P.table_request == 0, "n = %llu: asks for a table of %u copies", (unsigned long long)n, P.table_request);
    EXPECT(P.copies == 1, "n = %llu: %u copies", (unsigned long long)n, P.copies);
    EXPECT(P.terms == n && P.srs_n == n && P.shape.batch == batch && P.shape.pieces == 1 && P.shape.piece_terms == n, "n = %llu: terms / batch recorded", (unsigned long long)n);
    EXPECT(P.run != MSM_RUN_SHORT, "n = %llu: the short path needs the table", (unsigned long long)n);
    if (n == 0) {
        const MsmPlan Q = msm_plan_nothing(0, batch, 0);
        EXPECT(P.run == MSM_RUN_NOTHING && P.shape.path == PLK_MSM_PATH_EMPTY && !memcmp(&P, &Q, sizeof P), "zero terms");
        return;
    }
    if (n < MSM_NAIVE_BELOW) {
        MsmPlan Q = msm_plan_naive(n, batch, n);
        Q.table_request = 0;
        EXPECT(P.run == MSM_RUN_NAIVE && P.shape.path == PLK_MSM_PATH_NAIVE && P.shape.table_copies == 1 && !memcmp(&P, &Q, sizeof P), "n = %llu: not the naive plan", (unsigned long long)n);
        EXPECT(FITS32((n + MSM_THREADS - 1) / MSM_THREADS, P.grid_naive) && P.bytes_pinned == (size_t)batch * P.grid_naive * MSM_BYTES_XYZZ, "n = %llu: naive grid", (unsigned long long)n);
        return;
    }
    // the pass plan is msm_plan_pipeline for a key of `terms` points without shifted copies, alone on the context
    MsmPlan Q = msm_plan_pipeline(n, batch, n, 1, pick_window_bits(n, false), msm_index_bits(n), false, fused);
    Q.table_request = 0;
    EXPECT(!memcmp(&P, &Q, sizeof P), "n = %llu batch %u: not msm_plan_pipeline(terms, batch, terms, 1, pick_window_bits(terms, false), ..)", (unsigned long long)n, batch);
    const MsmParams &p = P.p;
    const uint32_t c = p.c;
    EXPECT(P.run == MSM_RUN_PIPELINE && P.shape.path == PLK_MSM_PATH_ORDINARY && P.shape.table_copies == 1, "n = %llu: path", (unsigned long long)n);
    EXPECT(c == (n < (1u << 17) ? 13u : n < (1u << 19) ? 15u : 17u) && P.shape.window_bits == c, "n = %llu: window bits %u", (unsigned long long)n, c);
    EXPECT(p.windows == 254 / c + 1 && p.groups == p.windows && P.shape.windows == p.windows && P.shape.bucket_sets == p.windows, "n = %llu: %u sets, %u windows", (unsigned long long)n, p.groups, p.windows);
    EXPECT(p.copy_stride == 0, "n = %llu: copy stride %u with one copy", (unsigned long long)n, p.copy_stride);
    EXPECT(p.fine_bits == FINE_BITS && P.shape.fine_bits == FINE_BITS && p.nbins == 1u << (c - 1 - FINE_BITS) && p.nbins <= 1024 && P.shape.coarse_bins == p.nbins, "n = %llu: %u bins", (unsigned long long)n, p.nbins);
    EXPECT(p.n == n && p.batch == batch && p.nbits == msm_index_bits(n) && (1ull << p.nbits) >= n && (1ull << p.nbits) <= MSM_PASS_MAX_TERMS, "n = %llu: n, batch, nbits", (unsigned long long)n);
    EXPECT(P.shape.prephase == 2, "n = %llu: the fused pre-phase needs ONE bucket set", (unsigned long long)n);
    EXPECT(P.shape.accumulate_variant == (n <= MSM_OWNED_MAX ? 2u : 0u), "n = %llu: variant %u", (unsigned long long)n, P.shape.accumulate_variant);
    EXPECT(P.shape.reduce_lanes == (batch >= 3 ? 16u : 32u), "n = %llu batch %u: %u lanes", (unsigned long long)n, batch, P.shape.reduce_lanes);
    // 64-bit restatement of every 32-bit product
    const uint64_t sets = (uint64_t)batch * p.groups, bins = sets * p.nbins, windows = (uint64_t)batch * p.windows;
    const uint64_t tasks = bins + windows * n / TASK_MAX + 1;
    EXPECT(FITS32(sets, P.total_sets) && FITS32(bins, P.total_bins) && FITS32(windows, P.total_windows) && FITS32(tasks, P.max_tasks), "n = %llu batch %u: totals truncated", (unsigned long long)n, batch);
    EXPECT(FITS32((tasks * (P.shape.reduce_lanes == 16 ? 16 : 32) + MSM_THREADS - 1) / MSM_THREADS, P.grid_reduce), "n = %llu: reduce grid truncated", (unsigned long long)n);
    EXPECT(FITS32((n + MSM_THREADS - 1) / MSM_THREADS, P.grid_digits) && FITS32((n + DIGIT_CHUNK - 1) / DIGIT_CHUNK, P.grid_partition), "n = %llu: pre-phase grids", (unsigned long long)n);
    EXPECT(windows * n <= 0xffffffffull, "n = %llu batch %u: entry offsets beyond 32 bits", (unsigned long long)n, batch);
    EXPECT(P.bytes_b == (size_t)(windows * n * 4) && P.bytes_f == (size_t)(windows * n * 4), "n = %llu: entries / digits", (unsigned long long)n);
    EXPECT(P.bytes_a == (size_t)((3 * bins + 4) * 4) && P.bytes_d == (size_t)(13 * sets * MSM_BYTES_XYZZ), "n = %llu: bytes_a / bytes_d", (unsigned long long)n);
    EXPECT(P.bytes_c == (size_t)(tasks * 2 * MSM_BYTES_XYZZW + tasks * meta_per_task(FINE_BITS) * 4) && P.bytes_e == (size_t)(tasks * slots_per_task(FINE_BITS) * MSM_BYTES_XYZZW), "n = %llu: task buffers", (unsigned long long)n);
    EXPECT(P.roles >= WS_FIRST_F_ROLE + 1 && P.bytes_pinned == (size_t)P.roles * sets * MSM_BYTES_XYZZ && P.roles <= 13, "n = %llu: %u roles (bytes_d holds 13 per set)", (unsigned long long)n, P.roles);
    EXPECT(P.lds_partition_scatter <= 96 * 1024 && P.lds_partition_count <= 64 * 1024, "n = %llu: LDS", (unsigned long long)n);
}

static int sweep_mode() {
    static const uint64_t edges[] = {0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 8195, 1u << 14, (1u << 16) - 1, 1u << 16, (1u << 16) + 1, (1u << 17) - 1, 1u << 17, (1u << 17) + 1,
                                     (1u << 19) - 1, 1u << 19, (1u << 19) + 1, 1u << 20, (1u << 22) + 12345, (1u << 24) - 1, 1u << 24};
    for (uint64_t n : edges)
        for (uint32_t batch = 1; batch <= MSM_MAX_BATCH; batch++)
            for (int fused = 0; fused < 2; fused++) check_pass(n, batch, fused != 0);
    for (uint64_t n = 3; n <= MSM_PASS_MAX_TERMS; n = n * 3 / 2 + 1)
        for (uint32_t batch = 1; batch <= MSM_MAX_BATCH; batch += 3) check_pass(n, batch, true);
    // the call: passes of 2^24 terms, one at a time
    static const uint64_t lengths[] = {0, 1, 4096, (1u << 24) - 1, 1u << 24, (1u << 24) + 1, 1u << 25, (1u << 25) + 1, 3u << 24, 1ull << 28, (1ull << 28) + 7, 1ull << 33};
    for (uint64_t n : lengths) {
        cases++;
        const MsmCallPlan C = msm_plan_bases_call(n);
        const uint64_t want = n ? (n + (1ull << 24) - 1) >> 24 : 1;
        EXPECT(C.piece_terms == MSM_PASS_MAX_TERMS && C.depth == 1 && C.pieces == want && C.pieces >= 1, "call of %llu terms: %llu pieces of %llu, depth %u", (unsigned long long)n,
               (unsigned long long)C.pieces, (unsigned long long)C.piece_terms, C.depth);
        EXPECT(C.pieces * C.piece_terms >= n && (C.pieces - 1) * C.piece_terms < (n ? n : 1), "call of %llu terms: the pieces do not tile it", (unsigned long long)n);
    }
    if (failures) { fprintf(stderr, "msm_bases_plan_check: %ld failures in %ld cases\n", failures, cases); return 1; }
    printf("msm_bases_plan_check: ok (%ld cases)\n", cases);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "table")) return table_mode();
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep_mode();
    fprintf(stderr, "usage: msm_bases_plan_check table|sweep\n");
    return 2;
}
