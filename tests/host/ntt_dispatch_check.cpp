// Stand-alone check of plonkit_amd/csrc/ntt_dispatch.h (which passes a scalar transform is given).  Built with -fsanitize=address,undefined by
// tests/test_ntt_dispatch_host.py and run directly.  Every decision comes from the header's functions.
//   ntt_dispatch_check plan      reads "log_n count inverse nonzero pre post tables" lines from stdin and prints the plan of each: one line
//                                "passes log_tile scratch_bytes d0 d1 d2 d3" and one line of the 23 fields of NttPassPlan per pass
//   ntt_dispatch_check kernels   reads "entry log_n count" lines (entry: ntt, intt, coset, icoset, lde4, lde4cm, icoset4cm — the library's entry points,
//                                tables allowed) and prints the kernel instantiations the entry's launches run, one line per input line
//   ntt_dispatch_check reachable prints every kernel instantiation any plan of the sweep's inputs names
//   ntt_dispatch_check batch     prints "rule log_n per" for the four batching rules and log_n 1..28
//   ntt_dispatch_check evict     reads "clock want cap count (key bytes used)*" lines and prints "compose" or "drop key*" for each
//   ntt_dispatch_check sweep     invariants of the plan over log_n x count x direction x nonzero x scalings x tables allowed
#include "../../plonkit_amd/csrc/ntt_dispatch.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace plk;

static std::string kernel_name(const NttPassPlan &q) {
    std::string s = q.role == NTT_ROLE_ROWS ? "rows" : "cols";
    if (q.family == NTT_FAMILY_BARRIER) return s + " B";
    s += " W<" + std::to_string(q.row_bits);
    if (q.log_tile != (uint32_t)NTT_LOG_TILE) s += ", " + std::to_string(q.log_tile);
    return s + ">";
}

static void print_plan(const NttPlan &P) {
    printf("%u %u %zu %u %u %u %u\n", P.passes, P.log_tile, P.scratch_bytes, P.digit[0], P.digit[1], P.digit[2], P.digit[3]);
    for (uint32_t i = 0; i < P.passes; i++) {
        const NttPassPlan &q = P.pass[i];
        printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", q.role, q.family, q.row_bits, q.log_tile, q.log_r, q.log_c, q.log_inner,
               q.log_r1, q.log_m1, q.log_m2, q.nonzero, q.quarter, q.pre, q.post, q.reads, q.writes, q.grid_x, q.block, q.lds_bytes, q.wants_table, q.table_bits,
               q.table_key, q.table_scaled);
    }
}

static int plan_mode() {
    unsigned log_n, count, inverse, pre, post, tables;
    unsigned long long nonzero;
    while (scanf("%u %u %u %llu %u %u %u", &log_n, &count, &inverse, &nonzero, &pre, &post, &tables) == 7) {
        if (log_n < 1 || log_n > MAX_LOG_N || count < 1 || count > NTT_MAX_BATCH) { fprintf(stderr, "bad line\n"); return 1; }
        print_plan(ntt_plan(log_n, count, inverse != 0, nonzero, pre, post, tables != 0));
    }
    return 0;
}

// the launches of one call of a library entry point (ntt.hip), tables allowed
static bool entry_plans(const char *entry, uint32_t log_n, uint32_t count, std::vector<NttPlan> &out) {
    const uint32_t N = NTT_SCALE_NONE, T = NTT_SCALE_TWO_LEVEL, E = NTT_SCALE_PER_ELEMENT;
    auto split = [&](uint32_t rule, uint32_t items, uint32_t each, auto plan) {
        const uint32_t per = ntt_batch_per_launch(rule, log_n);
        for (uint32_t done = 0; done < items; done += per) out.push_back(plan((items - done > per ? per : items - done) * each));
    };
    const bool direct = ntt_coset_direct_wanted(log_n, true);
    if (!strcmp(entry, "ntt")) split(NTT_BATCH_PLAIN, count, 1, [&](uint32_t b) { return ntt_plan(log_n, b, false, 0, N, N, true); });
    else if (!strcmp(entry, "intt")) split(NTT_BATCH_PLAIN, count, 1, [&](uint32_t b) { return ntt_plan(log_n, b, true, 0, N, N, true); });
    else if (!strcmp(entry, "coset")) split(NTT_BATCH_PLAIN, count, 1, [&](uint32_t b) { return ntt_plan(log_n, b, false, 0, T, N, true); });
    else if (!strcmp(entry, "icoset")) split(NTT_BATCH_PLAIN, count, 1, [&](uint32_t b) { return ntt_plan(log_n, b, true, 0, N, T, true); });
    else if (!strcmp(entry, "lde4")) split(NTT_BATCH_LDE4, count, 1, [&](uint32_t b) { return ntt_plan(log_n + 2, b, false, (uint64_t)1 << log_n, T, N, true); });
    else if (!strcmp(entry, "lde4cm")) split(NTT_BATCH_LDE4CM, count, 4, [&](uint32_t b) { return ntt_plan(log_n, b, false, 0, direct ? E : T, N, true); });
    else if (!strcmp(entry, "icoset4cm")) out.push_back(ntt_plan(log_n, 4, true, 0, N, direct ? E : T, true));
    else return false;
    return true;
}

static int kernels_mode() {
    char entry[32];
    unsigned log_n, count;
    while (scanf("%31s %u %u", entry, &log_n, &count) == 3) {
        std::vector<NttPlan> plans;
        if (log_n < 1 || log_n > MAX_LOG_N || count < 1 || !entry_plans(entry, log_n, count, plans)) { fprintf(stderr, "bad line\n"); return 1; }
        std::set<std::string> names;
        for (const NttPlan &P : plans) for (uint32_t i = 0; i < P.passes; i++) names.insert(kernel_name(P.pass[i]));
        bool first = true;
        for (const std::string &s : names) { printf("%s%s", first ? "" : "; ", s.c_str()); first = false; }
        printf("\n");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- the sweep
static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

template <class F> static void for_every_input(F f) {
    for (uint32_t log_n = 1; log_n <= MAX_LOG_N; log_n++)
        for (uint32_t count : {1u, 4u, 16u})
            for (int inverse = 0; inverse < 2; inverse++)
                for (uint64_t nonzero : {(uint64_t)0, ((uint64_t)1 << log_n) >> 2, ((uint64_t)1 << log_n) >> 1})
                    for (uint32_t pre = 0; pre < 3; pre++)
                        for (uint32_t post = 0; post < 3; post++)
                            for (int tables = 0; tables < 2; tables++) f(log_n, count, inverse != 0, nonzero, pre, post, tables != 0);
}

template <int LR, int LT> static bool tile_plan_exists() { return TilePlan<LR, LT>::SLOTS > 0; }       // instantiates the static_assert
static bool wave_kernel_exists(uint32_t row_bits, uint32_t log_tile, uint32_t role) {
    if (log_tile == (uint32_t)NTT_LOG_TILE) switch (row_bits) {
        case 7: return tile_plan_exists<7, NTT_LOG_TILE>();
        case 8: return tile_plan_exists<8, NTT_LOG_TILE>();
        case 9: return tile_plan_exists<9, NTT_LOG_TILE>();
        case 10: return tile_plan_exists<10, NTT_LOG_TILE>();
        default: return false;
    }
    // of the 4096-element tile ntt.hip builds the column pass of 11 row bits and the row pass of 10
    if (log_tile == (uint32_t)NTT_LOG_TILE_BIG) return role == NTT_ROLE_COLS ? (row_bits == 11 && tile_plan_exists<11, NTT_LOG_TILE_BIG>())
                                                                            : (row_bits == 10 && tile_plan_exists<10, NTT_LOG_TILE_BIG>());
    return false;
}

static int sweep_mode(bool print_reachable) {
    std::set<std::string> reachable;
    std::map<uint32_t, std::vector<uint32_t>> keys;            // table key -> (inverse, folded log_n, log_r, log_inner)
    size_t plans = 0;
    for_every_input([&](uint32_t log_n, uint32_t count, bool inverse, uint64_t nonzero, uint32_t pre, uint32_t post, bool tables) {
        const NttPlan P = ntt_plan(log_n, count, inverse, nonzero, pre, post, tables);
        const NttPlan Q = ntt_plan(log_n, count, inverse, nonzero, pre, post, tables);
        plans++;
        CHECK(!memcmp(&P, &Q, sizeof P), "log_n %u: two calls disagree", log_n);
        const uint64_t n = (uint64_t)1 << log_n;
        CHECK(P.passes >= 1 && P.passes <= NTT_MAX_PASSES, "log_n %u: %u passes", log_n, P.passes);
        CHECK(P.log_n == log_n && P.count == count && P.inverse == (inverse ? 1u : 0u), "log_n %u: the plan's own arguments", log_n);
        uint32_t sum = 0;
        for (uint32_t i = 0; i < 4; i++) {
            sum += P.digit[i];
            CHECK(P.digit[i] <= 11, "log_n %u: digit %u", log_n, P.digit[i]);
            CHECK((i < P.passes) == (P.digit[i] != 0), "log_n %u: digit %u of %u passes is %u", log_n, i, P.passes, P.digit[i]);
        }
        CHECK(sum == log_n, "log_n %u: digits sum to %u", log_n, sum);
        CHECK(P.scratch_bytes == (P.passes > 1 ? (size_t)count * n * 32 : 0), "log_n %u: scratch %zu", log_n, P.scratch_bytes);
        for (uint32_t i = 0; i < P.passes; i++) {
            const NttPassPlan &q = P.pass[i];
            const bool first = i == 0, last = i + 1 == P.passes;
            reachable.insert(kernel_name(q));
            CHECK(q.role == (last ? NTT_ROLE_ROWS : NTT_ROLE_COLS), "log_n %u pass %u: role", log_n, i);
            CHECK(q.log_r == P.digit[i], "log_n %u pass %u: log_r %u", log_n, i, q.log_r);
            CHECK((uint64_t)q.grid_x << (q.log_r + q.log_c) == n && q.grid_x >= 1, "log_n %u pass %u: grid %u of tiles 2^%u", log_n, i, q.grid_x, q.log_r + q.log_c);
            if (q.role == NTT_ROLE_COLS) {
                uint32_t rem = log_n;
                for (uint32_t j = 0; j <= i; j++) rem -= P.digit[j];
                CHECK(q.log_inner == rem, "log_n %u pass %u: log_inner %u", log_n, i, q.log_inner);
                CHECK(q.log_c <= q.log_inner, "log_n %u pass %u: log_c %u > log_inner %u", log_n, i, q.log_c, q.log_inner);
                CHECK(q.post == NTT_SCALE_NONE, "log_n %u pass %u: output scaling before the last pass", log_n, i);
            } else {
                CHECK(q.log_c <= q.log_r1, "log_n %u pass %u: log_c %u > log_r1 %u", log_n, i, q.log_c, q.log_r1);
                CHECK(q.log_r1 == (P.passes > 1 ? P.digit[0] : 0) && q.log_m1 == (P.passes > 2 ? P.digit[1] : 0) && q.log_m2 == 0, "log_n %u: digits of the last pass", log_n);
                CHECK(q.log_r1 + q.log_m1 + q.log_m2 + q.log_r == log_n, "log_n %u: the last pass's digits", log_n);
                CHECK(q.post == post && !q.wants_table, "log_n %u: last pass", log_n);
            }
            if (q.family == NTT_FAMILY_BARRIER) {
                // the closed trap: the barrier kernels hold at most 2^11 elements in 512 threads and the LDS their attribute allows
                CHECK(q.log_r + q.log_c <= 11, "log_n %u pass %u: a barrier pass of 2^%u elements", log_n, i, q.log_r + q.log_c);
                CHECK(q.lds_bytes == (36u << (q.log_r + q.log_c)), "log_n %u pass %u: lds", log_n, i);
                CHECK(q.lds_bytes <= (q.role == NTT_ROLE_ROWS ? NTT_LDS_ROWS : NTT_LDS_COLS), "log_n %u pass %u: %u B of LDS above the attribute", log_n, i, q.lds_bytes);
                CHECK(q.block == 512 && q.row_bits == 0 && q.log_tile == 0, "log_n %u pass %u: barrier launch", log_n, i);
            } else {
                CHECK(q.family == NTT_FAMILY_WAVE, "log_n %u pass %u: family", log_n, i);
                CHECK(wave_kernel_exists(q.row_bits, q.log_tile, q.role), "log_n %u pass %u: no ntt_pass_w<%u, %u, %u>", log_n, i, q.row_bits, q.role, q.log_tile);
                CHECK(q.row_bits == q.log_r && q.log_tile == q.log_r + q.log_c && q.log_tile == P.log_tile, "log_n %u pass %u: wave tile", log_n, i);
                CHECK(q.lds_bytes == (q.log_tile == 11 ? NTT_W_LDS : NTT_W_LDS_BIG) && q.block == (q.log_tile == 11 ? 512u : 1024u), "log_n %u pass %u: wave launch", log_n, i);
                CHECK(!(q.nonzero && q.pre == NTT_SCALE_PER_ELEMENT), "log_n %u pass %u: a wave pass with padding and a per-element table", log_n, i);
                CHECK(P.passes > 1, "log_n %u: a single wave pass", log_n);
            }
            CHECK(q.nonzero == (first ? (uint32_t)nonzero : 0) && q.pre == (first ? pre : (uint32_t)NTT_SCALE_NONE), "log_n %u pass %u: first-pass fields", log_n, i);
            CHECK(!q.quarter || (first && nonzero == n >> 2 && nonzero), "log_n %u pass %u: quarter", log_n, i);
            CHECK(q.reads == (first ? NTT_AT_SOURCE : NTT_AT_SCRATCH) && q.writes == (last ? NTT_AT_DATA : NTT_AT_SCRATCH), "log_n %u pass %u: reads / writes", log_n, i);
            const uint32_t bits = q.log_r + q.log_inner;
            CHECK(q.wants_table == ((tables && !last && bits > 14 && bits <= 25) ? 1u : 0u), "log_n %u pass %u: wants_table %u", log_n, i, q.wants_table);
            if (q.wants_table) {
                CHECK(q.table_bits == bits && q.table_scaled == ((inverse && first) ? 1u : 0u), "log_n %u pass %u: table", log_n, i);
                const std::vector<uint32_t> id = {inverse ? 1u : 0u, q.table_scaled ? log_n : 0, q.log_r, q.log_inner};
                auto it = keys.find(q.table_key);
                if (it == keys.end()) keys[q.table_key] = id;
                else CHECK(it->second == id, "log_n %u pass %u: key %08x names two tables", log_n, i, q.table_key);
            } else CHECK(!q.table_bits && !q.table_key && !q.table_scaled, "log_n %u pass %u: table fields without a table", log_n, i);
        }
        // the 4096-element tile: only with both passes wave-owned
        if (P.log_tile != 11) CHECK(P.log_tile == 12 && P.passes == 2 && P.pass[0].family == NTT_FAMILY_WAVE && P.pass[1].family == NTT_FAMILY_WAVE, "log_n %u: tile %u", log_n, P.log_tile);
        // has_scale: on inverse transforms, unless the first table has 1/n and was obtained
        CHECK(ntt_plan_has_scale(P, false) == (inverse ? 1u : 0u), "log_n %u: has_scale without the table", log_n);
        CHECK(ntt_plan_has_scale(P, true) == ((inverse && !P.pass[0].table_scaled) ? 1u : 0u), "log_n %u: has_scale with the table", log_n);
    });
    std::set<std::vector<uint32_t>> ids;
    for (auto &kv : keys) ids.insert(kv.second);
    CHECK(ids.size() == keys.size(), "%zu keys for %zu tables", keys.size(), ids.size());
    for (uint32_t log_n = 1; log_n <= MAX_LOG_N; log_n++)
        for (int t = 0; t < 2; t++) CHECK(ntt_coset_direct_wanted(log_n, t != 0) == (t && log_n > 14 && log_n <= 24), "coset tables at 2^%u", log_n);
    if (print_reachable) for (const std::string &s : reachable) printf("%s\n", s.c_str());
    else if (!fails) printf("ntt_dispatch_check: ok (%zu plans, %zu table keys)\n", plans, keys.size());
    return fails ? 1 : 0;
}

static int batch_mode() {
    for (uint32_t rule = 0; rule < 4; rule++)
        for (uint32_t log_n = 1; log_n <= MAX_LOG_N; log_n++) printf("%u %u %u\n", rule, log_n, ntt_batch_per_launch(rule, log_n));
    return 0;
}

static int evict_mode() {
    unsigned long long clock, want, cap;
    unsigned count;
    while (scanf("%llu %llu %llu %u", &clock, &want, &cap, &count) == 4) {
        std::vector<NttResident> res(count);
        for (unsigned i = 0; i < count; i++) {
            unsigned long long bytes, used;
            if (scanf("%u %llu %llu", &res[i].key, &bytes, &used) != 3) { fprintf(stderr, "bad line\n"); return 1; }
            res[i].bytes = bytes; res[i].used = used;
        }
        std::vector<uint32_t> drop(count);
        const int k = ntt_plan_eviction(res.data(), count, clock, want, cap, drop.data());
        if (k == NTT_EVICT_COMPOSE) { printf("compose\n"); continue; }
        if (k < 0 || (unsigned)k > count) { fprintf(stderr, "%d drops of %u tables\n", k, count); return 1; }
        printf("drop");
        for (int i = 0; i < k; i++) printf(" %u", drop[i]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "plan")) return plan_mode();
    if (!strcmp(mode, "kernels")) return kernels_mode();
    if (!strcmp(mode, "reachable")) return sweep_mode(true);
    if (!strcmp(mode, "batch")) return batch_mode();
    if (!strcmp(mode, "evict")) return evict_mode();
    if (!strcmp(mode, "sweep")) return sweep_mode(false);
    fprintf(stderr, "usage: ntt_dispatch_check plan|kernels|reachable|batch|evict|sweep\n");
    return 2;
}
