// Stand-alone check of the batch half of plonkit_amd/csrc/kzg_all_plan.h (plk_kzg_open_all_batch_dev, plk_g1_ntt_batch_dev): the limit of a
// launch, the scratch layout, the map from a flattened butterfly of a stage launch to (transform, butterfly), the two points a butterfly
// touches, and the gather of the first N points of every 2N block into the dense output.  The kernels of g1ntt.hip and kzg_all.hip call the
// same functions.  Built with -fsanitize=address,undefined and run directly (tests/test_kzg_all_batch_plan_host.py).
#include "../../plonkit_amd/csrc/kzg_all_plan.h"
#include <cstdio>
#include <vector>

using namespace plk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: %s — ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

int main() {
    // ---- the limit: count * 2^(log_n + 1) <= 2^26 for the openings, count << log_n <= 2^26 for the G1 batch; count >= 1
    EXPECT(FK_BATCH_LOG_POINTS == 26, "the limit of a launch is g1ntt's");
    for (uint32_t log_n = 0; log_n <= FK_MAX_LOG_N; log_n++) {
        const uint32_t most = 1u << (FK_BATCH_LOG_POINTS - 1 - log_n);                  // count * 2N = 2^26 exactly
        EXPECT(fk_batch_ok(1, log_n) && fk_batch_ok(most, log_n), "log_n %u: exactly 2^26 points were refused", log_n);
        EXPECT(!fk_batch_ok(most + 1, log_n), "log_n %u: one polynomial above the limit was accepted", log_n);
        EXPECT(!fk_batch_ok(0, log_n) && !fk_batch_ok(0xffffffffu, log_n), "log_n %u: count 0 or 2^32 - 1", log_n);
        EXPECT(fk_batch_points_ok(most, log_n + 1) && fk_batch_points_ok(2 * most, log_n) && !fk_batch_points_ok(2 * most + 1, log_n), "log_n %u: the G1 batch", log_n);
        // the byte arithmetic at the limit: 2^26 x 176 B does not fit 32 bits
        const FkScratch s = fk_batch_scratch(most, log_n, true);
        const size_t pts = (size_t)1 << FK_BATCH_LOG_POINTS;
        EXPECT(s.c_off == pts * FK_XYZZW_BYTES && s.coeff_off == pts * (FK_XYZZW_BYTES + FK_FR_BYTES) && s.bytes == s.coeff_off + pts / 2 * FK_FR_BYTES,
               "log_n %u: scratch at the limit %zu %zu %zu", log_n, s.c_off, s.coeff_off, s.bytes);
        EXPECT(s.bytes > 0xffffffffu, "log_n %u: the scratch at the limit is more than 32 bits hold", log_n);
    }
    EXPECT(!fk_batch_ok(1, 26) && !fk_batch_ok(2, 25) && fk_batch_ok(1, 25), "2^25 takes one polynomial");
    EXPECT(fk_batch_ok(1u << 13, 12) && !fk_batch_ok((1u << 13) + 1, 12), "2^12 takes 2^13 polynomials");
    EXPECT(fk_batch_points_ok(1, 26) && !fk_batch_points_ok(1, 27) && !fk_batch_points_ok(2, 26) && !fk_batch_points_ok(1, 0xffffffffu), "the G1 batch at 2^26");

    // ---- the scratch: three disjoint regions in order, 16-byte aligned, fk_scratch for count = 1
    const uint32_t counts[] = {1, 3, 37};
    for (uint32_t log_n = 0; log_n <= 12; log_n++) {
        const size_t n = (size_t)1 << log_n;
        for (int values = 0; values < 2; values++) {
            const FkScratch one = fk_scratch(log_n, values != 0), b1 = fk_batch_scratch(1, log_n, values != 0);
            EXPECT(one.u_off == b1.u_off && one.c_off == b1.c_off && one.coeff_off == b1.coeff_off && one.bytes == b1.bytes, "log_n %u: a batch of one is fk_scratch", log_n);
            for (uint32_t count : counts) {
                const FkScratch s = fk_batch_scratch(count, log_n, values != 0);
                const size_t u_end = s.u_off + count * 2 * n * FK_XYZZW_BYTES, c_end = s.c_off + count * 2 * n * FK_FR_BYTES;
                EXPECT(s.u_off == 0 && u_end <= s.c_off && c_end <= s.coeff_off, "log_n %u count %u: regions overlap", log_n, count);
                EXPECT(s.bytes == s.coeff_off + (values ? count * n * FK_FR_BYTES : 0), "log_n %u count %u: total", log_n, count);
                EXPECT(s.u_off % 16 == 0 && s.c_off % 16 == 0 && s.coeff_off % 16 == 0, "log_n %u count %u: alignment", log_n, count);
            }
        }
    }

    // ---- a stage launch: the butterfly map is a bijection onto (transform, butterfly); both points of a butterfly lie in the first 2^log_n of
    // the transform's own stride block (stride N: the public G1 batch; stride 2N: the N-point pass over the scratch of the openings); every
    // point of every transform is touched exactly once per stage
    for (uint32_t log_n = 1; log_n <= 9; log_n++) {
        const uint32_t n = 1u << log_n, half = n / 2;
        for (uint32_t count : counts) {
            std::vector<uint8_t> seen((size_t)count * half, 0);
            for (uint32_t g = 0; g < count * half; g++) {
                const FkButterfly b = fk_batch_butterfly(log_n, g);
                EXPECT(b.poly < count && b.j < half, "log_n %u count %u: butterfly %u -> (%u, %u)", log_n, count, g, b.poly, b.j);
                if (b.poly < count && b.j < half) seen[(size_t)b.poly * half + b.j]++;
                EXPECT(b.poly == g / half && b.j == g % half, "log_n %u count %u: the polynomial is not the slow index at %u", log_n, count, g);
            }
            for (size_t k = 0; k < seen.size(); k++) EXPECT(seen[k] == 1, "log_n %u count %u: (%zu, %zu) hit %u times", log_n, count, k / half, k % half, seen[k]);
            for (uint32_t stride : {n, 2 * n}) {
                for (uint32_t s = 0; s < log_n; s++) {
                    std::vector<uint8_t> touched((size_t)count * stride, 0);
                    for (uint32_t g = 0; g < count * half; g++) {
                        const FkButterfly b = fk_batch_butterfly(log_n, g);
                        const FkPair p = fk_stage_pair(log_n, s, b.j);
                        EXPECT(p.i0 < p.i1 && p.i1 < n && p.i1 - p.i0 == (1u << s) && p.jl < (1u << s) && (p.i0 & ((1u << s) - 1)) == p.jl,
                               "log_n %u stage %u: butterfly %u -> %u %u jl %u", log_n, s, b.j, p.i0, p.i1, p.jl);
                        const size_t a0 = (size_t)b.poly * stride + p.i0, a1 = (size_t)b.poly * stride + p.i1;
                        EXPECT(a0 / stride == b.poly && a1 / stride == b.poly && a1 < touched.size(), "log_n %u stage %u stride %u: butterfly %u leaves its block", log_n, s, stride, g);
                        if (a1 < touched.size()) { touched[a0]++; touched[a1]++; }
                    }
                    for (size_t a = 0; a < touched.size(); a++)
                        EXPECT(touched[a] == (a % stride < n ? 1 : 0), "log_n %u count %u stage %u stride %u: point %zu touched %u times", log_n, count, s, stride, a, touched[a]);
                }
            }
            // the gather into the dense output reads the first N of every block, each once, in order
            for (uint32_t stride : {n, 2 * n}) {
                for (uint32_t p = 0; p < count * n; p++) {
                    const uint32_t src = fk_batch_point(log_n, stride, p);
                    EXPECT(src == (p / n) * stride + p % n && src % stride < n && src / stride == p / n, "log_n %u count %u stride %u: output %u reads %u", log_n, count, stride, p, src);
                }
            }
        }
    }
    // log_n = 0 has no stage; its gather is one point per block
    for (uint32_t p = 0; p < 37; p++) EXPECT(fk_batch_point(0, 2, p) == 2 * p && fk_batch_point(0, 1, p) == p, "log_n 0: output %u", p);
    // the last point of a launch at the limit keeps inside 32 bits
    EXPECT(fk_batch_point(25, 1u << 26, (1u << 25) - 1) == (1u << 25) - 1 && fk_batch_point(12, 1u << 13, (1u << 25) - 1) == (1u << 26) - (1u << 12) - 1, "the last output at the limit");
    const FkButterfly last = fk_batch_butterfly(13, (1u << 25) - 1);
    EXPECT(last.poly == (1u << 13) - 1 && last.j == (1u << 12) - 1, "the last butterfly at the limit");

    if (failures) { fprintf(stderr, "kzg_all_batch_plan_check: %d failures\n", failures); return 1; }
    printf("kzg_all_batch_plan_check: ok\n");
    return 0;
}
