// AddressSanitizer + UndefinedBehaviorSanitizer build of the .wtns container check (wtns_container, circuit.cpp: no HIP in it) — what
// plk_wtns_decode and plk_prove_wtns run on a client's bytes before anything reaches the device.  gcc, no GPU, the recipe of
// sanitize_host.cpp: the host translation units are compiled in directly, the two symbols they take from the device half are provided
// here.  Input: one .wtns file, then every truncation of its head, every single-byte overwrite of its 76 container bytes and a few thousand
// random mutations.  Every call must return, an accepted container must lie inside the buffer (payload + 32 n <= len), and whatever
// wtns_container accepts or refuses, parse_wtns_bin (plk_circuit_load's parser) must accept or refuse with the same words.  Built and run
// by tests/test_wtns_sanitizer.py.
#include "../../plonkit_amd/csrc/circuit.cpp"
#include "../../plonkit_amd/csrc/hostapi.cpp"
#include <cstdio>
#include <fstream>

namespace plk {
static thread_local std::string g_err;
void set_error(const std::string &m) { g_err = m; }
}
extern "C" const char *plk_last_error(void) { return plk::g_err.c_str(); }
void plk_circuit_unregister(plk_circuit *) {}

static uint64_t rs = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }

static int accepted = 0, refused = 0, disagreements = 0;
static void check(const std::vector<uint8_t> &in) {
    // an exact-size heap copy: one byte read behind the end is a report
    std::unique_ptr<uint8_t[]> b(new uint8_t[in.size() ? in.size() : 1]);
    if (!in.empty()) memcpy(b.get(), in.data(), in.size());
    uint64_t n = 0; size_t payload = 0;
    plk::g_err.clear();
    const bool ok = plk::wtns_container(b.get(), in.size(), &n, &payload);
    const std::string words = plk::g_err;
    if (ok && (payload > in.size() || n > (in.size() - payload) / 32)) { fprintf(stderr, "accepted container exceeds the buffer\n"); exit(1); }
    plk::big_vector<plk::HFr> out;
    plk::g_err.clear();
    const bool ok2 = plk::parse_wtns_bin(b.get(), in.size(), &out);
    if (ok ? !(ok2 ? out.size() == n : plk::g_err == "read witness failed: not in field") : (ok2 || plk::g_err != words)) disagreements++;
    if (ok) accepted++; else refused++;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: sanitize_wtns file.wtns iterations\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<uint8_t> good((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int iters = atoi(argv[2]);
    check(good);
    if (!accepted) { fprintf(stderr, "the untouched file was refused: %s\n", plk_last_error()); return 1; }
    for (size_t cut = 0; cut < good.size() && cut <= 120; cut++) check(std::vector<uint8_t>(good.begin(), good.begin() + cut));
    for (size_t off = 0; off < 76 && off < good.size(); off++)
        for (int v : {0x00, 0x01, 0x7f, 0x80, 0xff}) { std::vector<uint8_t> b = good; b[off] = (uint8_t)v; check(b); }
    for (int it = 0; it < iters; it++) {
        std::vector<uint8_t> b = good;
        switch (rnd() % 4) {
            case 0: b[rnd() % 76 % b.size()] ^= (uint8_t)(1u << (rnd() % 8)); break;
            case 1: b.resize(rnd() % (b.size() + 1)); break;
            case 2: { size_t o = rnd() % 76 % b.size(); uint32_t v = (uint32_t)rnd(); for (size_t i = 0; i < 4 && o + i < b.size(); i++) b[o + i] = (uint8_t)(v >> (8 * i)); break; }
            default: { size_t o = rnd() % b.size(); for (size_t i = 0; i < 32 && o + i < b.size(); i++) b[o + i] = 0xff; }
        }
        check(b);
    }
    check(std::vector<uint8_t>());
    printf("sanitize_wtns: %d accepted, %d refused, %d disagreements\n", accepted, refused, disagreements);
    return disagreements ? 1 : 0;
}
