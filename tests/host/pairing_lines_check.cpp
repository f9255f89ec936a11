// The Miller loop from the host-built line table (pairing.cpp miller_lines, what plk_vk_load uploads) against miller_loop itself, coefficient
// for coefficient: for each 256-byte G2 pair named on the command line, both points, at G1 = infinity and at i * G for i = 1..10.  Also the
// number of lines (64 + popcount + 2) and a G2 point at infinity.  gcc, no HIP, no GPU.  Driver: tests/test_pairing_lines_host.py.
#include "../../plonkit_amd/csrc/pairing.cpp"
#include <cstdio>
#include <vector>

using namespace plk::host;

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: pairing_lines_check g2pair.bin...\n"); return 2; }
    int bad = 0, checks = 0;
    const int n = miller_line_count();
    if (n != 64 + __builtin_popcountll(ate_loop_lo()) + 2 || ate_loop_lo() != 11347224129447541672ULL) { printf("line count %d\n", n); bad++; }
    HAffine G; G.x = HFq::from_u64(1); G.y = HFq::from_u64(2);
    std::vector<HAffine> ps;
    { HAffine O; O.x = HFq::zero(); O.y = HFq::zero(); ps.push_back(O); }
    { HJac acc = HJac::inf(); for (int i = 1; i <= 10; i++) { acc = jac_add(acc, jac_from_affine(G)); ps.push_back(jac_to_affine(acc)); } }
    for (int f = 1; f < argc; f++) {
        uint8_t b[256];
        FILE *fp = fopen(argv[f], "rb");
        if (!fp || fread(b, 1, 256, fp) != 256) { fprintf(stderr, "%s: cannot read 256 bytes\n", argv[f]); return 2; }
        fclose(fp);
        for (int q = 0; q < 2; q++) {
            G2Affine Q;
            if (!g2_from_bytes(b + 128 * q, &Q)) { fprintf(stderr, "%s: G2 point %d not on the twist\n", argv[f], q); return 2; }
            std::vector<Fq2> lines((size_t)2 * n);
            miller_lines(Q, lines.data());
            for (size_t i = 0; i < ps.size(); i++) {
                const Fq12 want = miller_loop_value(ps[i], Q), got = miller_loop_from_lines(ps[i], lines.data(), Q.inf);
                checks++;
                for (int k = 0; k < 12; k++) if (!(want.c[k] == got.c[k])) { printf("%s point %d, G1 %zu: coefficient %d differs\n", argv[f], q, i, k); bad++; break; }
                if (i == 0 && !got.is_one()) { printf("infinity must give 1\n"); bad++; }
                if (i > 0 && got.is_one()) { printf("a Miller value of 1 for a finite point\n"); bad++; }
            }
        }
    }
    {   // Q at infinity: 1 whatever the table holds
        G2Affine Q; Q.inf = true; Q.x = Fq2::zero(); Q.y = Fq2::zero();
        std::vector<Fq2> lines((size_t)2 * n, Fq2::zero());
        checks++;
        if (!miller_loop_from_lines(ps[3], lines.data(), true).is_one() || !miller_loop_value(ps[3], Q).is_one()) { printf("Q = infinity must give 1\n"); bad++; }
    }
    printf("%d lines per point, %d checks, %d mismatches\n", n, checks, bad);
    return bad ? 1 : 0;
}
