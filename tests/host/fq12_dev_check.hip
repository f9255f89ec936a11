// The device pairing check of plonkit_amd/csrc/fq12_dev.h compiled for the HOST (its functions are __host__ __device__) against the host
// pairing of pairing.cpp: for pairs (A, B) = (-42 b G + e G, b G) and the G2 pair {G2, 42 G2} of the tau = 42 key the product
// e(A, Q0) e(B, Q1) is 1 exactly when e = 0, and the shortened final exponentiation must say what pairing_product_is_one says,
// also with either G1 argument at infinity and with a G2 point at infinity.  No GPU involved.  Driver: tests/test_fq12_dev_host.py.
#include "../../plonkit_amd/csrc/pairing.cpp"
#include "../../plonkit_amd/csrc/pairing_table.h"
#include <cstdio>

using namespace plk;
using namespace plk::host;

static HAffine mulG(uint64_t k) {
    HAffine G; G.x = HFq::from_u64(1); G.y = HFq::from_u64(2);
    const uint64_t c[4] = {k, 0, 0, 0};
    return jac_to_affine(jac_mul(jac_from_affine(G), c));
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: fq12_dev_check g2.bin\n"); return 2; }
    uint8_t g2b[256];
    FILE *fp = fopen(argv[1], "rb");
    if (!fp || fread(g2b, 1, 256, fp) != 256) { fprintf(stderr, "cannot read 256 bytes of G2\n"); return 2; }
    fclose(fp);
    G2Affine g2[2];
    if (!g2_from_bytes(g2b, &g2[0]) || !g2_from_bytes(g2b + 128, &g2[1])) { fprintf(stderr, "G2 not on the twist\n"); return 2; }
    int bad = 0, cases = 0, ones = 0;
    auto check = [&](const HAffine &a, const HAffine &b, const G2Affine q[2], const char *what) {
        PairingHead head; std::vector<Fq> lines;
        make_pairing_table(q, &head, &lines);
        const HAffine g1s[2] = {a, b};
        const bool want = pairing_product_is_one(g1s, q, 2);
        const bool got = pairing_is_one_from_lines(fq_of(a.x), fq_of(a.y), fq_of(b.x), fq_of(b.y), &head, lines.data());
        cases++; ones += want;
        if (want != got) { bad++; printf("MISMATCH %s: host %d device-code %d\n", what, (int)want, (int)got); }
    };
    HAffine O; O.x = HFq::zero(); O.y = HFq::zero();
    for (uint64_t b = 1; b <= 4; b++) {
        const HAffine B = mulG(b * 7919), A = mulG(42 * b * 7919);
        HAffine An = A; An.y = -A.y;
        check(An, B, g2, "true pair");
        check(A, B, g2, "sign off");
        check(mulG(42 * b * 7919 + 1), B, g2, "off by one");
    }
    check(O, O, g2, "(O, O)");
    check(O, mulG(5), g2, "(O, B)");
    check(mulG(5), O, g2, "(A, O)");
    {   // a G2 point at infinity: its factor is 1
        G2Affine q[2] = {g2[0], g2[1]}; q[1].inf = true;
        check(O, mulG(9), q, "Q1 infinity, A = O");
        check(mulG(9), mulG(9), q, "Q1 infinity");
        q[0].inf = true;
        check(mulG(9), mulG(11), q, "both infinity");
    }
    {   // the same point twice: e(A, Q) e(-A, Q) = 1
        G2Affine q[2] = {g2[1], g2[1]};
        HAffine A = mulG(123456789), An = A; An.y = -A.y;
        check(A, An, q, "same Q");
        check(A, A, q, "same Q, not inverse");
    }
    printf("%d cases, %d are one, %d mismatches\n", cases, ones, bad);
    return bad ? 1 : 0;
}
