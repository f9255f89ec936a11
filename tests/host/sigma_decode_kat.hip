// Host run of sigma_decode (plonkit_amd/csrc/sigma_decode_dev.h): the per-value routine the kernel k_sigma_decode calls, compiled for the
// CPU and applied to the cases tests/test_copy_cases_host.py writes — every log_n from 1 to 26, labels of all four cosets and the values
// the decode must refuse.  No GPU is touched (hipcc only compiles).
//
//   sigma_decode_kat <cases> <results>
//   cases:   32 B omega_{2^28}, 32 B its inverse (Montgomery limbs), u32 count, then count x { u32 log_n, 32 B value as stored }
//   results: count x u32 (col << 30 | row, or 0xFFFFFFFF)
// The powers of omega come from pow_u64 here, not from the context's tables: the routine takes them through a callable.
#include <cstdio>
#include <cstring>
#include <vector>
#include "sigma_decode_dev.h"

using namespace plk;

struct PowOf {
    Fr base;
    Fr operator()(uint32_t e) const { return pow_u64(base, e); }
};

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: sigma_decode_kat <cases> <results>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    Fr root, root_inv;
    uint32_t count = 0;
    if (!read_all(in, root.l, 32) || !read_all(in, root_inv.l, 32) || !read_all(in, &count, 4)) { fprintf(stderr, "short header\n"); return 2; }
    if (mul(root, root_inv) != Fr::one()) { fprintf(stderr, "the two roots are not inverse to each other\n"); return 2; }
    std::vector<uint32_t> out(count);
    SigmaConsts C[SIGMA_MAX_LOG_N + 1];
    bool have[SIGMA_MAX_LOG_N + 1] = {false};
    for (uint32_t i = 0; i < count; i++) {
        uint32_t log_n;
        Fr x;
        if (!read_all(in, &log_n, 4) || !read_all(in, x.l, 32)) { fprintf(stderr, "short case %u\n", i); return 2; }
        if (log_n < 1 || log_n > SIGMA_MAX_LOG_N) { fprintf(stderr, "case %u: log_n %u\n", i, log_n); return 2; }
        if (!have[log_n]) { C[log_n] = sigma_consts(log_n); have[log_n] = true; }
        out[i] = sigma_decode(x, log_n, C[log_n], PowOf{root}, PowOf{root_inv});
    }
    fclose(in);
    FILE *of = fopen(argv[2], "wb");
    if (!of) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), 4, count, of) != count) { fprintf(stderr, "short write\n"); return 2; }
    fclose(of);
    printf("%u values decoded on the host\n", count);
    return 0;
}
