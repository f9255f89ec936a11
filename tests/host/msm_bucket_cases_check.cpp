// Stand-alone check of the bucket schedule's integer rules (plonkit_amd/csrc/msm_plan.h, "the bucket schedule": the functions the kernels
// msm_scan_bins, msm_accumulate, msm_fold_hot, msm_task_reduce, msm_task_reduce_quad and msm_bin_fold call).  Built with
// -fsanitize=address,undefined by tests/test_msm_bucket_cases_host.py and run directly.
//   msm_bucket_cases_check table   reads cases from stdin and prints what the rules make of them:
//        in:   case <name> <build> <variant>            variant 2: the build with the owned rule
//              bin <exact> <64 bucket populations>      exact 1: the populations of every task of the bin are known (one task, or one bucket)
//              end
//        out:  case <name> <build>
//              bin <j> count <entries> tasks <k> folded <0|1>
//              task <j> <slice> nc <nc> mu <mu> owned <0|1|-1> max <fullest bucket|-1> idle <lanes without entries> short <entries of the last live lane>
//              bucket <j> <slice> <fine> <entries> <empty|primary|walked|folded> <tf> <tl> <span>     (exact tasks; as the reducers class it)
//   msm_bucket_cases_check slices  count = 1 .. 5 * CHUNK: the slices of a bin are non-empty, sum to count, none exceeds CHUNK
//   msm_bucket_cases_check spans   random populations: a bucket's entries lie in the pieces of lanes tf .. tl and in no others
#include "../../plonkit_amd/csrc/msm_plan.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace plk;

static const uint32_t FINE = 1u << FINE_BITS;
static const char *CLASSES[4] = {"empty", "primary", "walked", "folded"};        // MSM_BUCKET_*
static long failures = 0, cases = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures++ < 40) { fprintf(stderr, "FAIL %s:%d: %s — ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// one task whose bucket populations are known: what msm_accumulate writes into its meta and what the reducers make of every bucket
static void print_task(int j, uint32_t slice, const uint32_t *cnt, int variant, bool exact) {
    uint32_t nc = 0, max_cnt = 0;
    for (uint32_t f = 0; f < FINE; f++) { nc += cnt[f]; max_cnt = cnt[f] > max_cnt ? cnt[f] : max_cnt; }
    const uint32_t mu = msm_lane_entries(nc);
    const bool owned = variant == 2 && exact && msm_task_owned(max_cnt, mu);
    uint32_t idle = 0, short_piece = 0;
    for (uint32_t tid = 0; tid < (uint32_t)MSM_THREADS; tid++) {
        const uint32_t lo = msm_lane_lo(tid, mu, nc), hi = msm_lane_hi(lo, mu, nc);
        if (lo >= hi) idle++; else short_piece = hi - lo;
    }
    printf("task %d %u nc %u mu %u owned %d max %d idle %u short %u\n", j, slice, nc, mu, exact ? (int)owned : -1, exact ? (int)max_cnt : -1, idle, short_piece);
    if (!exact) return;
    const uint32_t mu_reduce = owned ? 0x7fffffffu : (nc ? mu : 1);             // (msm_task_reduce: an owned task's buckets are whole)
    uint32_t s0 = 0;
    for (uint32_t f = 0; f < FINE; f++) {
        const uint32_t e0 = s0 + cnt[f], cls = msm_bucket_class(s0, e0, mu_reduce);
        if (cls != MSM_BUCKET_EMPTY)
            printf("bucket %d %u %u %u %s %u %u %u\n", j, slice, f, cnt[f], CLASSES[cls], msm_bucket_first_lane(s0, mu_reduce), msm_bucket_last_lane(e0, mu_reduce),
                   msm_bucket_span(s0, e0, mu_reduce));
        else printf("bucket %d %u %u 0 empty 0 0 0\n", j, slice, f);
        s0 = e0;
    }
}

static int table_mode() {
    char word[64], name[128], build[64];
    int variant = 0, bins = 0;
    while (scanf("%63s", word) == 1) {
        if (!strcmp(word, "case")) {
            if (scanf("%127s %63s %d", name, build, &variant) != 3) return 1;
            printf("case %s %s\n", name, build);
            bins = 0; cases++;
        } else if (!strcmp(word, "bin")) {
            int exact;
            uint32_t cnt[64], count = 0, occupied = 0;
            if (scanf("%d", &exact) != 1) return 1;
            for (uint32_t f = 0; f < FINE; f++) { if (scanf("%u", &cnt[f]) != 1) return 1; count += cnt[f]; occupied += cnt[f] != 0; }
            const uint32_t k = msm_bin_tasks(count);
            printf("bin %d count %u tasks %u folded %d\n", bins, count, k, (int)msm_bin_folded(k));
            if (exact && k > 1 && occupied != 1) { fprintf(stderr, "%s: a bin of %u tasks is exact only with ONE bucket\n", name, k); return 1; }
            for (uint32_t s = 0; s < k; s++) {
                const uint32_t len = msm_slice_len(count, k, s);
                uint32_t part[64];
                for (uint32_t f = 0; f < FINE; f++) part[f] = k == 1 ? cnt[f] : (exact && cnt[f] ? len : 0);
                if (!exact) { memset(part, 0, sizeof part); part[0] = len; }          // (only nc, mu and the lanes are printed)
                print_task(bins, s, part, variant, exact != 0);
            }
            bins++;
        } else if (strcmp(word, "end")) { fprintf(stderr, "unknown word %s\n", word); return 1; }
    }
    fprintf(stderr, "msm_bucket_cases_check: %ld cases\n", cases);
    return 0;
}

static int slices_mode() {
    for (uint32_t count = 1; count <= 5 * CHUNK; count++) {
        cases++;
        const uint32_t k = msm_bin_tasks(count), per = msm_slice_per(count, k);
        EXPECT(k >= 1 && (uint64_t)k * CHUNK >= count && (uint64_t)(k - 1) * CHUNK < count, "count %u: %u tasks", count, k);
        uint32_t sum = 0, at = 0;
        for (uint32_t s = 0; s < k; s++) {
            const uint32_t b = msm_slice_begin(0, count, per, s), e = msm_slice_end(b, count, per), len = msm_slice_len(count, k, s);
            EXPECT(b == at && e > b && len == e - b && len <= CHUNK, "count %u slice %u of %u: [%u, %u) after %u", count, s, k, b, e, at);
            EXPECT(s + 1 == k || len == per, "count %u slice %u: %u entries, not the last slice", count, s, len);
            sum += len; at = e;
        }
        EXPECT(sum == count && at == count, "count %u: the slices hold %u", count, sum);
        EXPECT(msm_bin_folded(k) == (k >= 5), "count %u: %u tasks folded %d", count, k, (int)msm_bin_folded(k));
    }
    if (failures) { fprintf(stderr, "msm_bucket_cases_check slices: %ld failures\n", failures); return 1; }
    printf("msm_bucket_cases_check slices: ok (%ld cases)\n", cases);
    return 0;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t below) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 20) % below);
}

// the lanes a bucket's entries REALLY fall into, entry by entry from the cut into pieces, against (tf, tl) and the class
static void check_spans(const uint32_t *cnt) {
    cases++;
    uint32_t nc = 0;
    for (uint32_t f = 0; f < FINE; f++) nc += cnt[f];
    if (!nc) return;
    const uint32_t mu = msm_lane_entries(nc);
    EXPECT(mu >= 1 && (uint64_t)mu * MSM_THREADS >= nc && (uint64_t)(mu - 1) * MSM_THREADS < nc, "nc %u: mu %u", nc, mu);
    std::vector<uint32_t> lane_of(nc, 0xffffffffu);
    uint32_t covered = 0;
    for (uint32_t tid = 0; tid < (uint32_t)MSM_THREADS; tid++) {
        const uint32_t lo = msm_lane_lo(tid, mu, nc), hi = msm_lane_hi(lo, mu, nc);
        EXPECT(lo <= hi && hi <= nc && hi - lo <= mu, "nc %u lane %u: [%u, %u)", nc, tid, lo, hi);
        for (uint32_t i = lo; i < hi; i++) { EXPECT(lane_of[i] == 0xffffffffu, "nc %u: entry %u in two pieces", nc, i); lane_of[i] = tid; covered++; }
    }
    EXPECT(covered == nc, "nc %u: the pieces hold %u entries", nc, covered);
    uint32_t s0 = 0;
    for (uint32_t f = 0; f < FINE; f++) {
        const uint32_t e0 = s0 + cnt[f], cls = msm_bucket_class(s0, e0, mu);
        if (!cnt[f]) { EXPECT(cls == MSM_BUCKET_EMPTY && msm_bucket_span(s0, e0, mu) == 0, "nc %u bucket %u: empty but class %u", nc, f, cls); continue; }
        const uint32_t tf = msm_bucket_first_lane(s0, mu), tl = msm_bucket_last_lane(e0, mu), span = msm_bucket_span(s0, e0, mu);
        EXPECT(lane_of[s0] == tf && lane_of[e0 - 1] == tl && span == tl - tf, "nc %u mu %u bucket %u [%u, %u): lanes %u .. %u, rule %u .. %u", nc, mu, f, s0, e0, lane_of[s0],
               lane_of[e0 - 1], tf, tl);
        for (uint32_t i = s0; i < e0; i++) EXPECT(lane_of[i] >= tf && lane_of[i] <= tl, "nc %u bucket %u: entry %u in lane %u", nc, f, i, lane_of[i]);
        for (uint32_t t = tf; t <= tl; t++) {                                   // every lane of tf .. tl holds some of it
            const uint32_t lo = msm_lane_lo(t, mu, nc), hi = msm_lane_hi(lo, mu, nc);
            EXPECT(lo < e0 && hi > s0, "nc %u bucket %u: lane %u of %u .. %u holds none of it", nc, f, t, tf, tl);
        }
        const uint32_t want = tf == tl ? MSM_BUCKET_PRIMARY : (tl - tf > HOT_SPAN ? MSM_BUCKET_FOLDED : MSM_BUCKET_WALKED);
        EXPECT(cls == want && msm_span_folded(span) == (cls == MSM_BUCKET_FOLDED), "nc %u bucket %u: class %u, lanes %u .. %u", nc, f, cls, tf, tl);
    }
}

static int spans_mode() {
    for (int round = 0; round < 4000; round++) {
        uint32_t cnt[64];
        const uint32_t shape = rnd(4), cap = shape == 0 ? 4 : shape == 1 ? 40 : shape == 2 ? 256 : 2 * (CHUNK / 64);
        uint32_t nc = 0;
        for (uint32_t f = 0; f < FINE; f++) { cnt[f] = rnd(3) == 0 ? 0 : rnd(cap + 1); nc += cnt[f]; }
        if (round % 7 == 0) cnt[rnd(64)] += rnd(CHUNK / 2);                    // a hot bucket
        nc = 0;
        for (uint32_t f = 0; f < FINE; f++) nc += cnt[f];
        for (uint32_t f = 0; nc > CHUNK; f = (f + 1) % FINE) { const uint32_t cut = cnt[f] < nc - CHUNK ? cnt[f] : nc - CHUNK; cnt[f] -= cut; nc -= cut; }
        check_spans(cnt);
    }
    if (failures) { fprintf(stderr, "msm_bucket_cases_check spans: %ld failures\n", failures); return 1; }
    printf("msm_bucket_cases_check spans: ok (%ld cases)\n", cases);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "table")) return table_mode();
    if (argc == 2 && !strcmp(argv[1], "slices")) return slices_mode();
    if (argc == 2 && !strcmp(argv[1], "spans")) return spans_mode();
    fprintf(stderr, "usage: msm_bucket_cases_check table|slices|spans\n");
    return 2;
}
