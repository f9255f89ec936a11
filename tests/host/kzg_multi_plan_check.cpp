// Stand-alone check of plonkit_amd/csrc/kzg_multi_plan.h (the host algebra of the multi-point openings, kzg_multi.hip).
// Reads cases from standard input — "m p gamma u", the p points, the m masks, the m x p evaluations, scalars in hexadecimal — and prints
// for each: the verdict on the sets, the weights w_ij, the matrix gamma^i w_ij, c_i followed by Z_T(u), and r_i(u);
// tests/test_kzg_multi_host.py compares the lines with the Python-integer model (tests/gen/kzg_multi_cases.py).  What needs no model
// is checked here: the refusals of malformed sets, and the kernels' constants (powers of the point, 0^0 = 1).
// Built with -fsanitize=address,undefined and run directly.
#include "../../plonkit_amd/csrc/kzg_multi_plan.h"
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
    // the refusals, in the header's order
    {
        const HFr pts[3] = {HFr::from_u64(5), HFr::from_u64(6), HFr::from_u64(7)}, dup[3] = {pts[0], pts[1], pts[0]};
        const uint32_t ok[3] = {1, 2, 4}, empty[3] = {1, 0, 6}, above[3] = {1, 2, 12}, unused[3] = {1, 2, 3};
        EXPECT(km_check_sets(pts, 3, ok, 3) == KM_SETS_OK, "well-formed sets");
        EXPECT(km_check_sets(dup, 3, ok, 3) == KM_SETS_DUPLICATE_POINT, "duplicate point");
        EXPECT(km_check_sets(pts, 3, empty, 3) == KM_SETS_EMPTY, "empty set");
        EXPECT(km_check_sets(pts, 3, above, 3) == KM_SETS_BIT_ABOVE, "bit above");
        EXPECT(km_check_sets(pts, 3, unused, 3) == KM_SETS_UNUSED_POINT, "unused point");
        EXPECT(km_check_sets(pts, 0, ok, 3) == KM_SETS_COUNTS && km_check_sets(pts, 9, ok, 3) == KM_SETS_COUNTS, "points out of range");
        EXPECT(km_check_sets(pts, 3, ok, 0) == KM_SETS_COUNTS && km_check_sets(pts, 3, ok, 33) == KM_SETS_COUNTS, "polynomials out of range");
    }
    // the kernels' constants: t^e, t^(8 * 2^s), t^2048, (t^2048)^(per * 2^s), all times 32; zero is an ordinary point
    {
        const HFr w32 = HFr::from_u64(32);
        for (uint64_t tv : {0ull, 1ull, 3ull, 0xfffffffffffffffull}) {
            const HFr t = HFr::from_u64(tv);
            for (uint32_t tiles : {1u, 2u, 256u, 257u, 131072u}) {
                HFr c[KM_CONSTS];
                km_point_constants(t, tiles, c);
                const uint32_t per = km_chunk(tiles);
                EXPECT(per * KM_THREADS >= tiles && (per - 1) * KM_THREADS < tiles, "chunk of %u tiles", tiles);
                for (uint32_t e = 0; e < KM_EPT; e++) EXPECT(c[KM_C_POW + e] == t.pow_u64(e) * w32, "t^%u", e);
                for (uint32_t s = 0; s < KM_LOG_THREADS; s++) {
                    EXPECT(c[KM_C_LANE + s] == t.pow_u64(8ull << s) * w32, "lane step %u", s);
                    EXPECT(c[KM_C_CHUNK + s] == t.pow_u64(2048ull * per << s) * w32, "chunk step %u of %u tiles", s, tiles);
                }
                EXPECT(c[KM_C_TILE] == t.pow_u64(2048) * w32, "tile step");
                if (tv == 0) EXPECT(c[KM_C_POW] == w32 && c[KM_C_POW + 1].is_zero() && c[KM_C_TILE].is_zero(), "0^0 = 1 and nothing else");
            }
        }
        EXPECT(km_tiles(1) == 1 && km_tiles(2048) == 1 && km_tiles(2049) == 2 && km_tiles(1ull << 28) == 131072, "tiles");
    }
    int cases = 0;
    if (scanf("%d", &cases) != 1) cases = 0;
    for (int k = 0; k < cases; k++) {
        unsigned m = 0, p = 0;
        if (scanf("%u %u", &m, &p) != 2 || m == 0 || m > KM_MAX_OPEN || p == 0 || p > KM_MAX_POINTS) { fprintf(stderr, "bad case header\n"); return 2; }
        const HFr gamma = read_fr(), u = read_fr();
        std::vector<HFr> pts(p), y((size_t)m * p), w((size_t)m * p), mat((size_t)m * p), c(m);
        std::vector<uint32_t> sets(m);
        for (auto &t : pts) t = read_fr();
        for (auto &s : sets) if (scanf("%u", &s) != 1) return 2;
        for (auto &v : y) v = read_fr();
        printf("sets %d\n", km_check_sets(pts.data(), p, sets.data(), m));
        km_weights(pts.data(), p, sets.data(), m, w.data());
        km_matrix(w.data(), gamma, m, p, mat.data());
        HFr z_t;
        km_c(pts.data(), p, sets.data(), m, gamma, u, c.data(), &z_t);
        printf("w"); for (const auto &v : w) print_fr(v); printf("\n");
        printf("m"); for (const auto &v : mat) print_fr(v); printf("\n");
        printf("c"); for (const auto &v : c) print_fr(v); print_fr(z_t); printf("\n");
        printf("r"); for (unsigned i = 0; i < m; i++) print_fr(km_r_at(pts.data(), p, sets[i], w.data() + (size_t)i * p, y.data() + (size_t)i * p, u)); printf("\n");
        // Z of the whole set times Z of the rest is Z_T
        for (unsigned i = 0; i < m; i++) EXPECT(km_z(pts.data(), p, sets[i], u) * km_z(pts.data(), p, ((1u << p) - 1) & ~sets[i], u) == z_t, "case %d polynomial %u", k, i);
    }
    if (failures) { fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    printf("kzg_multi_plan_check: ok\n");
    return 0;
}
