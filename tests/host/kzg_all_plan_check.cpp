// Stand-alone check of plonkit_amd/csrc/kzg_all_plan.h (the index maps, sizes and limits of the one-pass openings, kzg_all.hip).
// The two views of each arrangement are held against each other here — where coefficient i and key point j land, and what stands at
// position m — together with the limits and the scratch layout; the maps themselves are printed for log_n = 0 .. 12, one line each, and
// tests/test_kzg_all_plan_host.py compares them with the Python-integer model (tests/gen/fk20_cases.py).
// Built with -fsanitize=address,undefined and run directly.
#include "../../plonkit_amd/csrc/kzg_all_plan.h"
#include <cstdio>
#include <vector>

using namespace plk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: %s — ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

int main() {
    for (uint32_t log_n = 0; log_n <= 12; log_n++) {
        const uint32_t n = 1u << log_n, n2 = 2 * n;
        std::vector<long> c(n2), t(n2);
        for (uint32_t m = 0; m < n2; m++) {
            const uint32_t cs = fk_c_source(log_n, m), ts = fk_t_source(log_n, m);
            c[m] = cs == FK_NONE ? -1 : (long)cs;
            t[m] = ts == FK_NONE ? -1 : (long)ts;
            EXPECT(cs == FK_NONE || (cs >= 1 && cs < n), "log_n %u: c[%u] reads coefficient %u", log_n, m, cs);
            EXPECT(ts == FK_NONE || ts + 2 <= n, "log_n %u: t[%u] reads key point %u beyond N - 2", log_n, m, ts);
            EXPECT(ts == FK_NONE || ts < fk_key_points_needed(log_n), "log_n %u: t[%u] reads a point the key-length rule does not cover", log_n, m);
        }
        // from the side of the inputs: every coefficient but f_0 and every key point 0 .. N - 2 lands exactly where the other view finds it
        EXPECT(fk_c_index_of_coeff(0) == FK_NONE, "f_0 enters c");
        uint32_t c_used = 0, t_used = 0;
        for (uint32_t i = 1; i < n; i++) { const uint32_t m = fk_c_index_of_coeff(i); EXPECT(m < n2 && c[m] == (long)i, "log_n %u: coefficient %u", log_n, i); c_used++; }
        for (uint32_t j = 0; j + 2 <= n; j++) { const uint32_t m = fk_t_index_of_key(log_n, j); EXPECT(m < n2 && t[m] == (long)j, "log_n %u: key point %u", log_n, j); t_used++; }
        uint32_t c_set = 0, t_set = 0;
        for (uint32_t m = 0; m < n2; m++) { c_set += c[m] >= 0; t_set += t[m] >= 0; }
        EXPECT(c_set == c_used && t_set == t_used, "log_n %u: %u / %u positions of c, %u / %u of t are set", log_n, c_set, c_used, t_set, t_used);
        printf("C %u", log_n);
        for (uint32_t m = 0; m < n2; m++) printf(" %ld", c[m]);
        printf("\nT %u", log_n);
        for (uint32_t m = 0; m < n2; m++) printf(" %ld", t[m]);
        printf("\n");
    }
    // the limits
    EXPECT(fk_size_ok(0) && fk_size_ok(25) && !fk_size_ok(26) && !fk_size_ok(0xffffffffu), "sizes: 2^25 is the last one accepted");
    EXPECT(FK_MAX_LOG_N == 25, "FK_MAX_LOG_N");
    for (uint32_t log_n = 0; log_n <= 25; log_n++) {
        const uint64_t n = (uint64_t)1 << log_n;
        EXPECT(fk_key_points_needed(log_n) == n - 1, "log_n %u: points needed", log_n);
        if (n >= 2) EXPECT(!fk_key_ok(log_n, n - 2), "log_n %u: a key of N - 2 points was accepted", log_n);
        EXPECT(fk_key_ok(log_n, n - 1) && fk_key_ok(log_n, n) && fk_key_ok(log_n, n + 1), "log_n %u: a key of N - 1 or N points was refused", log_n);
        // the scratch: the three parts do not overlap, every part is 16-byte aligned, nothing is wasted
        for (int values = 0; values < 2; values++) {
            const FkScratch s = fk_scratch(log_n, values != 0);
            EXPECT(s.u_off == 0 && s.c_off == 2 * n * FK_XYZZW_BYTES && s.coeff_off == s.c_off + 2 * n * FK_FR_BYTES, "log_n %u: layout", log_n);
            EXPECT(s.bytes == s.coeff_off + (values ? n * FK_FR_BYTES : 0), "log_n %u: total", log_n);
            EXPECT(s.c_off % 16 == 0 && s.coeff_off % 16 == 0, "log_n %u: alignment", log_n);
        }
        EXPECT(fk_key_transform_bytes(log_n) == 2 * n * FK_XYZZW_BYTES, "log_n %u: the key's transform", log_n);
    }
    EXPECT(fk_key_ok(0, 0), "N = 1 reads no key point");
    EXPECT(FK_XYZZW_BYTES == 144 && FK_AFFINE_BYTES == 64 && FK_FR_BYTES == 32 && FK_KEEP_BYTES == ((size_t)64 << 20), "constants");
    if (failures) { fprintf(stderr, "kzg_all_plan_check: %d failures\n", failures); return 1; }
    printf("kzg_all_plan_check: ok\n");
    return 0;
}
