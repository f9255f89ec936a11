// AddressSanitizer + UndefinedBehaviorSanitizer build of the host half of plk_verify_many: plk_verify_terms (verify.cpp) and the line-table
// builder (pairing.cpp miller_lines) over the golden vk.bin / proof.bin, a truncated proof, a proof of the wrong input count, and every
// prefix length of the proof.  gcc, no HIP, no GPU, its own main, no preloaded runtime.  Driver: tests/test_verify_many_sanitizer.py.
#include "../../plonkit_amd/csrc/hostapi.cpp"
#include "../../plonkit_amd/csrc/pairing.cpp"
#include "../../plonkit_amd/csrc/verify.cpp"
#include <cstdio>
#include <fstream>
#include <memory>

namespace plk {
static thread_local std::string g_err;
void set_error(const std::string &m) { g_err = m; }
}
extern "C" const char *plk_last_error(void) { return plk::g_err.c_str(); }

static std::vector<uint8_t> slurp(const char *p) { std::ifstream f(p, std::ios::binary); return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: sanitize_verify_many vk.bin proof.bin\n"); return 2; }
    const std::vector<uint8_t> vk = slurp(argv[1]), proof = slurp(argv[2]);
    int bad = 0;
    plk_g1_affine pts[25]; plk_fr sc[25]; int32_t early = -1, valid = -1;
    // the golden pair: terms, and the verifier agrees
    if (plk_verify_terms(vk.data(), vk.size(), proof.data(), proof.size(), 0, pts, sc, &early) != PLK_OK || early != 1) { printf("golden: rc / early\n"); bad++; }
    if (plk_verify_ex(vk.data(), vk.size(), proof.data(), proof.size(), 0, &valid) != PLK_OK || valid != 1) { printf("golden: verify\n"); bad++; }
    // truncated proof, every prefix: refused with the verifier's words, nothing read past the end (the copy has exactly `len` bytes)
    for (size_t len = 0; len < proof.size(); len++) {
        std::unique_ptr<uint8_t[]> cut(new uint8_t[len]);                // exactly len bytes, and not null at len = 0
        memcpy(cut.get(), proof.data(), len);
        const int32_t rc = plk_verify_terms(vk.data(), vk.size(), cut.get(), len, 0, pts, sc, &early);
        if (rc != PLK_ERR_ARG || plk::g_err != "plk_verify: malformed proof") { printf("prefix %zu: rc %d (%s)\n", len, rc, plk::g_err.c_str()); bad++; break; }
    }
    {   // one more public input than the key has: a verdict, settled before any group arithmetic
        std::vector<uint8_t> more(proof.begin(), proof.begin() + 8);
        uint64_t n_in = 0; for (int i = 0; i < 8; i++) n_in = (n_in << 8) | proof[8 + i];
        const uint64_t n2 = n_in + 1;
        for (int i = 7; i >= 0; i--) more.push_back((uint8_t)(n2 >> (8 * i)));
        more.insert(more.end(), proof.begin() + 16, proof.begin() + 16 + 32 * n_in);
        more.insert(more.end(), 32, 0);
        more.insert(more.end(), proof.begin() + 16 + 32 * n_in, proof.end());
        const int32_t rc = plk_verify_terms(vk.data(), vk.size(), more.data(), more.size(), 0, pts, sc, &early);
        if (rc != PLK_OK || early != 0) { printf("wrong input count: rc %d early %d\n", rc, early); bad++; }
        if (plk_verify_ex(vk.data(), vk.size(), more.data(), more.size(), 0, &valid) != PLK_OK || valid != 0) { printf("wrong input count: verify\n"); bad++; }
    }
    {   // truncated key, unknown flag, null
        if (plk_verify_terms(vk.data(), vk.size() - 1, proof.data(), proof.size(), 0, pts, sc, &early) != PLK_ERR_ARG) { printf("short key\n"); bad++; }
        if (plk_verify_terms(vk.data(), vk.size(), proof.data(), proof.size(), 8, pts, sc, &early) != PLK_ERR_ARG) { printf("flag\n"); bad++; }
        if (plk_verify_terms(vk.data(), vk.size(), proof.data(), proof.size(), 0, nullptr, sc, &early) != PLK_ERR_ARG) { printf("null\n"); bad++; }
    }
    {   // the line tables of the key's G2 pair, and the loop from them
        using namespace plk::host;
        const int n = miller_line_count();
        HAffine P; P.x = HFq::from_u64(1); P.y = HFq::from_u64(2);
        for (int q = 0; q < 2; q++) {
            G2Affine Q;
            if (!g2_from_bytes(vk.data() + vk.size() - 256 + 128 * q, &Q)) { printf("g2 %d\n", q); bad++; continue; }
            std::vector<Fq2> lines((size_t)2 * n);
            miller_lines(Q, lines.data());
            const Fq12 a = miller_loop_value(P, Q), b = miller_loop_from_lines(P, lines.data(), false);
            for (int k = 0; k < 12; k++) if (!(a.c[k] == b.c[k])) { printf("lines %d: coefficient %d\n", q, k); bad++; break; }
        }
    }
    printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
