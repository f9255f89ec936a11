// Stand-alone check of plonkit_amd/csrc/kzg_multi_values_plan.h (the host algebra of the multi-point openings from values,
// kzg_multi_values.hip).  Reads cases from standard input — "log_n m p gamma u", the p points, the m masks, the m x p evaluations, the
// m x p sums S_ij, scalars in hexadecimal — and prints for each: which points lie on the domain, -(t^N - 1) / N per point, (N - 1) / 2,
// g_j = sum_i gamma^i w_ij y_ij, the value at k_j of term j for the points on the domain (0 off it), and sum_i c_i r_i(u);
// tests/test_kzg_multi_values_host.py compares the lines with the Python-integer model (tests/gen/kzg_multi_values_cases.py).
// What needs no model is checked here: the lane layout of the sums kernel, (N - 1) / 2 against the sum it stands for on a small domain.
// Built with -fsanitize=address,undefined and run directly.
#include "../../plonkit_amd/csrc/kzg_multi_values_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace plk::host;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: %s — ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static HFr read_fr() {
    char word[80];
    if (scanf("%79s", word) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    uint64_t c[4] = {0, 0, 0, 0};
    const size_t len = strlen(word);
    for (size_t k = 0; k < len; k++) {
        const char ch = word[len - 1 - k];
        const uint64_t d = ch <= '9' ? ch - '0' : ch - 'a' + 10;
        if (k < 64) c[k / 16] |= d << (4 * (k % 16));
    }
    return HFr::from_canonical(c);
}
static void print_fr(const HFr &v) {
    uint64_t c[4];
    v.to_canonical(c);
    printf(" %016llx%016llx%016llx%016llx", (unsigned long long)c[3], (unsigned long long)c[2], (unsigned long long)c[1], (unsigned long long)c[0]);
}

int main() {
    // the lanes of the sums kernel: pairs x slices lanes are busy, never more than the workgroup has, and a lone pair takes them all
    for (uint32_t pairs = 1; pairs <= KM_THREADS; pairs++) {
        const uint32_t s = kml_slices(pairs);
        EXPECT(s >= 1 && pairs * s <= KM_THREADS && pairs * (s + 1) > KM_THREADS, "%u pairs", pairs);
    }
    EXPECT(kml_slices(1) == KM_THREADS && kml_slices(KM_THREADS) == 1 && kml_slices(129) == 1 && kml_slices(128) == 2, "slices at the ends");
    // (N - 1) / 2 is the sum over the rest of the domain, whichever point is left out; 7 generates the 2^28-th roots of unity
    {
        uint64_t e[4] = {0x43e1f593f0000000ull >> 28 | (0x2833e84879b97091ull << 36), 0x2833e84879b97091ull >> 28 | (0xb85045b68181585dull << 36),
                         0xb85045b68181585dull >> 28 | (0x30644e72e131a029ull << 36), 0x30644e72e131a029ull >> 28};      // (r - 1) / 2^28
        const HFr root28 = HFr::from_u64(7).pow(e);
        EXPECT(root28.pow_u64(1ull << 28) == HFr::one() && root28.pow_u64(1ull << 27) != HFr::one(), "7^((r - 1) / 2^28) has order 2^28");
        for (uint32_t log_n : {1u, 2u, 5u}) {
            const uint32_t n = 1u << log_n;
            const HFr w = root28.pow_u64(1ull << (28 - log_n));
            for (uint32_t k : {0u, 1u, n - 1}) {
                const HFr t = w.pow_u64(k);
                EXPECT(kml_on_domain(t, log_n), "omega^%u at 2^%u", k, log_n);
                HFr sum = HFr::zero();
                for (uint32_t x = 0; x < n; x++) if (x != k) sum = sum + w.pow_u64(x) * (w.pow_u64(x) - t).inv();
                EXPECT(sum == kml_rest_sum(log_n), "rest of the domain without %u at 2^%u", k, log_n);
            }
            EXPECT(!kml_on_domain(HFr::zero(), log_n) && !kml_on_domain(HFr::from_u64(42), log_n), "0 and 42 are off the domain");
            EXPECT(kml_eval_scale(HFr::zero(), log_n) == HFr::from_u64(n).inv(), "the scale at 0 is 1 / N");
            EXPECT(kml_eval_scale(w, log_n).is_zero(), "the scale vanishes on the domain");
        }
    }
    int cases = 0;
    if (scanf("%d", &cases) != 1) cases = 0;
    for (int k = 0; k < cases; k++) {
        unsigned log_n = 0, m = 0, p = 0;
        if (scanf("%u %u %u", &log_n, &m, &p) != 3 || log_n == 0 || log_n > 28 || m == 0 || m > KM_MAX_OPEN || p == 0 || p > KM_MAX_POINTS) { fprintf(stderr, "bad case header\n"); return 2; }
        const HFr gamma = read_fr(), u = read_fr();
        std::vector<HFr> pts(p), y((size_t)m * p), S((size_t)m * p), w((size_t)m * p), mat((size_t)m * p), c(m), g(p);
        std::vector<uint32_t> sets(m);
        for (auto &t : pts) t = read_fr();
        for (auto &s : sets) if (scanf("%u", &s) != 1) return 2;
        for (auto &v : y) v = read_fr();
        for (auto &v : S) v = read_fr();
        EXPECT(km_check_sets(pts.data(), p, sets.data(), m) == KM_SETS_OK, "case %d: well-formed sets", k);
        km_weights(pts.data(), p, sets.data(), m, w.data());
        km_matrix(w.data(), gamma, m, p, mat.data());
        HFr z_t;
        km_c(pts.data(), p, sets.data(), m, gamma, u, c.data(), &z_t);
        kml_g(mat.data(), y.data(), m, p, g.data());
        printf("on"); for (const auto &t : pts) printf(" %d", kml_on_domain(t, log_n) ? 1 : 0); printf("\n");
        printf("scale"); for (const auto &t : pts) print_fr(kml_eval_scale(t, log_n)); printf("\n");
        printf("rest"); print_fr(kml_rest_sum(log_n)); printf("\n");
        printf("g"); for (const auto &v : g) print_fr(v); printf("\n");
        printf("at");
        for (unsigned j = 0; j < p; j++) {
            HFr ms = HFr::zero();
            for (unsigned i = 0; i < m; i++) ms = ms + mat[(size_t)i * p + j] * S[(size_t)i * p + j];
            print_fr(kml_on_domain(pts[j], log_n) ? kml_at_domain_point(pts[j], ms, g[j], log_n) : HFr::zero());
        }
        printf("\n");
        printf("v"); print_fr(kml_value_at_u(pts.data(), p, sets.data(), m, c.data(), w.data(), y.data(), u)); printf("\n");
    }
    if (failures) { fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    printf("kzg_multi_values_plan_check: ok\n");
    return 0;
}
