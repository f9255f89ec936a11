// The host side of a key set (plonkit_amd/csrc/vkset_plan.h: table deduplication, image layout, key-index validation, compaction) and the
// lookup every lane of the mixed kernels goes through (vkset_dev.h vkset_lookup, __host__ __device__), run on the CPU on images built in heap
// blocks of exactly their own length, so that the sanitizer build of this same program reports a read past the end.  Then the front lane
// code (verify_front_dev.h) per key THROUGH the lookup against verify_terms_parsed.  No GPU involved.  Driver: tests/test_verify_mixed_host.py.
//
//   verify_mixed_check vkA.bin vkF.bin proofA.bin proofF.bin      two keys that differ in n only, and a proof that verifies under each
#include "../../plonkit_amd/csrc/hostapi.cpp"
#include "../../plonkit_amd/csrc/pairing.cpp"
#include "../../plonkit_amd/csrc/verify.cpp"
#include "../../plonkit_amd/csrc/verify_front_dev.h"
#include "../../plonkit_amd/csrc/pairing_table.h"
#include "../../plonkit_amd/csrc/vkset_dev.h"
#include <cstdio>
#include <fstream>
#include <memory>

namespace plk {
static thread_local std::string g_err;
void set_error(const std::string &m) { g_err = m; }
}
extern "C" const char *plk_last_error(void) { return plk::g_err.c_str(); }

using namespace plk;

typedef std::vector<uint8_t> Bytes;
static Bytes slurp(const std::string &p) { std::ifstream f(p, std::ios::binary); return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }

static int bad = 0, checks = 0;
#define EXPECT(cond) do { checks++; if (!(cond)) { bad++; if (bad < 30) printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

// ---------------------------------------------------------------------------------------------- deduplication
static void dedup_cases() {
    const uint32_t n = 7;
    Bytes g2((size_t)n * VKSET_G2_BYTES);
    for (size_t i = 0; i < g2.size(); i++) g2[i] = (uint8_t)(i % VKSET_G2_BYTES * 7 + 1);       // all seven equal
    std::vector<uint32_t> table_of, first;
    EXPECT(vkset_dedup(g2.data(), n, &table_of, &first) == 1 && first == std::vector<uint32_t>({0}) && table_of == std::vector<uint32_t>(n, 0));
    // one differing byte, at the first, a middle and the last position of the 256, makes a second table
    for (size_t at : {(size_t)0, (size_t)127, (size_t)128, (size_t)255}) {
        Bytes h = g2;
        h[3 * VKSET_G2_BYTES + at] ^= 1;
        EXPECT(vkset_dedup(h.data(), n, &table_of, &first) == 2);
        EXPECT(first == std::vector<uint32_t>({0, 3}) && table_of == std::vector<uint32_t>({0, 0, 0, 1, 0, 0, 0}));
    }
    {   // tables in order of first appearance; equal bytes far apart share one
        Bytes h = g2;
        h[1 * VKSET_G2_BYTES + 5] = 0xaa; h[4 * VKSET_G2_BYTES + 5] = 0xaa; h[2 * VKSET_G2_BYTES + 200] = 0xbb; h[6 * VKSET_G2_BYTES + 200] = 0xbb; h[5 * VKSET_G2_BYTES] = 0xcc;
        EXPECT(vkset_dedup(h.data(), n, &table_of, &first) == 4);
        EXPECT(first == std::vector<uint32_t>({0, 1, 2, 5}) && table_of == std::vector<uint32_t>({0, 1, 2, 0, 1, 3, 2}));
    }
    {   // every key its own table; a single key
        Bytes h = g2;
        for (uint32_t k = 0; k < n; k++) h[(size_t)k * VKSET_G2_BYTES + 255] = (uint8_t)(100 + k);
        EXPECT(vkset_dedup(h.data(), n, &table_of, &first) == n);
        for (uint32_t k = 0; k < n; k++) EXPECT(table_of[k] == k && first[k] == k);
        EXPECT(vkset_dedup(h.data(), 1, &table_of, &first) == 1 && table_of.size() == 1 && table_of[0] == 0);
    }
}

// ---------------------------------------------------------------------------------------------- layout
static void layout_cases() {
    const size_t real = sizeof(PairingHead) + (size_t)host::miller_line_count() * 8 * sizeof(Fq);
    for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 7u, 64u, 1023u, VKSET_MAX_KEYS}) for (uint32_t T : {1u, 2u, 5u}) for (size_t tb : {real, real + 1, real + 15, (size_t)16}) {
        if (T > n) continue;
        const VksetLayout L = vkset_layout(n, T, tb);
        EXPECT(L.n_keys == n && L.n_tables == T);
        EXPECT(L.front_off == 0 && L.fixed_off == (size_t)n * sizeof(FrontVk) && L.index_off == L.fixed_off + (size_t)n * 12 * sizeof(G1Affine));
        EXPECT(L.tables_off >= L.index_off + (size_t)n * 4 && L.tables_off < L.index_off + (size_t)n * 4 + 16);
        EXPECT(L.table_stride >= tb && L.table_stride < tb + 16);
        EXPECT(L.bytes == L.tables_off + (size_t)T * L.table_stride);
        EXPECT((L.front_off | L.fixed_off | L.index_off | L.tables_off | L.table_stride | L.bytes) % 16 == 0);
    }
}

// ---------------------------------------------------------------------------------------------- key indices and compaction
static void index_cases() {
    uint64_t at = 77;
    EXPECT(vkset_indices_ok(nullptr, 0, 1, &at) && at == 77);
    std::vector<uint32_t> k = {0, 2, 1, 2, 0};
    EXPECT(vkset_indices_ok(k.data(), k.size(), 3, &at) && at == 77);
    EXPECT(!vkset_indices_ok(k.data(), k.size(), 2, &at) && at == 1);          // the lowest bad one
    k[4] = 3;
    EXPECT(!vkset_indices_ok(k.data(), k.size(), 3, &at) && at == 4);
    k[4] = UINT32_MAX; k[0] = UINT32_MAX;
    EXPECT(!vkset_indices_ok(k.data(), k.size(), VKSET_MAX_KEYS, &at) && at == 0);
    EXPECT(vkset_indices_ok(k.data() + 1, 3, 3, &at));

    const uint8_t mark[9] = {0xff, 0, 2, 0xff, 0xff, 2, 0, 0xff, 1};
    const uint32_t key[9] = {4, 9, 9, 0, 7, 9, 9, 4, 9};
    std::vector<uint64_t> live = {123}; std::vector<uint32_t> live_key = {456};
    vkset_compact(mark, key, 9, &live, &live_key);
    EXPECT(live == std::vector<uint64_t>({0, 3, 4, 7}) && live_key == std::vector<uint32_t>({4, 0, 7, 4}));
    vkset_compact(mark + 1, key + 1, 2, &live, &live_key);
    EXPECT(live.empty() && live_key.empty());
    vkset_compact(mark, key, 0, &live, &live_key);
    EXPECT(live.empty() && live_key.empty());
    vkset_compact(mark + 3, key + 3, 2, &live, &live_key);                     // all survive
    EXPECT(live == std::vector<uint64_t>({0, 1}) && live_key == std::vector<uint32_t>({0, 7}));
}

// ---------------------------------------------------------------------------------------------- the lookup on a synthetic image
static void lookup_cases() {
    for (uint32_t n : {1u, 3u, 5u, 64u}) for (uint32_t T : {1u, 2u, 3u}) {
        if (T > n) continue;
        const size_t tb = sizeof(PairingHead) + 88 * 8 * sizeof(Fq) + 8;       // a length that is no multiple of 16
        const VksetLayout L = vkset_layout(n, T, tb);
        std::unique_ptr<uint8_t[]> img(new uint8_t[L.bytes]);
        memset(img.get(), 0, L.bytes);
        for (uint32_t k = 0; k < n; k++) { const uint32_t t = (k * 7 + 1) % T; memcpy(img.get() + L.index_off + 4 * (size_t)k, &t, 4); }
        const VksetView v = vkset_view(img.get(), L);
        EXPECT(v.n_keys == n && v.n_tables == T && v.table_stride == L.table_stride);
        for (uint32_t k = 0; k < n; k++) {
            VksetKey key;
            EXPECT(vkset_lookup(v, k, &key));
            const uint8_t *tab = img.get() + L.tables_off + (size_t)((k * 7 + 1) % T) * L.table_stride;
            EXPECT((const uint8_t *)key.front == img.get() + L.front_off + (size_t)k * sizeof(FrontVk));
            EXPECT((const uint8_t *)key.fixed == img.get() + L.fixed_off + (size_t)k * 12 * sizeof(G1Affine));
            EXPECT((const uint8_t *)key.head == tab && (const uint8_t *)key.lines == tab + sizeof(PairingHead));
            EXPECT((const uint8_t *)key.head + tb <= img.get() + L.bytes);       // the whole table lies inside the image
            EXPECT(((uintptr_t)key.front | (uintptr_t)key.fixed | (uintptr_t)key.head | (uintptr_t)key.lines) % 16 == (uintptr_t)img.get() % 16);
        }
        VksetKey key; memset(&key, 0x5a, sizeof key);
        const VksetKey before = key;
        for (uint32_t k : {n, n + 1, n + 63, 0x80000000u, UINT32_MAX - 1, UINT32_MAX}) {
            EXPECT(!vkset_lookup(v, k, &key));
            EXPECT(memcmp(&key, &before, sizeof key) == 0);                        // "out of range" writes nothing
        }
        const uint32_t wild = T;                                                   // an image that names a table it does not hold
        memcpy(img.get() + L.index_off, &wild, 4);
        EXPECT(!vkset_lookup(v, 0, &key));
    }
}

// ---------------------------------------------------------------------------------------------- the front lane code per key, through the lookup
struct HostKey {
    ParsedVk *parsed = nullptr;
    FrontVk front;
    plk_g1_affine fixed[VERIFY_FIXED];
    host::G2Affine g2[2];
    Bytes g2_bytes;
    HostKey(const Bytes &vk, uint32_t flags) {
        parsed = parsed_vk_new(vk.data(), vk.size());
        if (!parsed) { fprintf(stderr, "verification key does not parse\n"); exit(2); }
        plk_fr nr[3], om;
        memset(&front, 0, sizeof front);
        parsed_vk_front(parsed, &front.n, &front.num_inputs, nr, &om);
        front.flags = flags;
        memcpy(front.non_residues, nr, sizeof nr); memcpy(&front.omega, &om, 32);
        parsed_vk_points(parsed, fixed, g2);
        g2_bytes.assign(vk.end() - VKSET_G2_BYTES, vk.end());
    }
    ~HostKey() { parsed_vk_free(parsed); }
    HostKey(const HostKey &) = delete;
};

static void front_cases(const Bytes &vkA, const Bytes &vkF, const Bytes &proofA, const Bytes &proofF) {
    const HostKey A(vkA, 0), F(vkF, 0);
    const HostKey *keys[3] = {&A, &F, &A};                                         // key 2 repeats key 0
    const uint32_t n = 3;
    Bytes g2;
    for (const HostKey *k : keys) g2.insert(g2.end(), k->g2_bytes.begin(), k->g2_bytes.end());
    std::vector<uint32_t> table_of, first;
    const uint32_t T = vkset_dedup(g2.data(), n, &table_of, &first);
    EXPECT(T == 1);                                                                // A and F differ in n only
    PairingHead head; std::vector<Fq> lines;
    make_pairing_table(A.g2, &head, &lines);
    EXPECT(head.lines == (uint32_t)host::miller_line_count() && lines.size() == (size_t)head.lines * 8);
    const VksetLayout L = vkset_layout(n, T, sizeof head + lines.size() * sizeof(Fq));
    std::unique_ptr<uint8_t[]> img(new uint8_t[L.bytes]);
    memset(img.get(), 0, L.bytes);
    for (uint32_t k = 0; k < n; k++) {
        memcpy(img.get() + L.front_off + (size_t)k * sizeof(FrontVk), &keys[k]->front, sizeof(FrontVk));
        memcpy(img.get() + L.fixed_off + (size_t)k * sizeof keys[k]->fixed, keys[k]->fixed, sizeof keys[k]->fixed);
        memcpy(img.get() + L.index_off + 4 * (size_t)k, &table_of[k], 4);
    }
    memcpy(img.get() + L.tables_off, &head, sizeof head);
    memcpy(img.get() + L.tables_off + sizeof head, lines.data(), lines.size() * sizeof(Fq));
    const VksetView v = vkset_view(img.get(), L);

    const Bytes *proofs[2] = {&proofA, &proofF};
    int went_on = 0, settled = 0;
    for (int pi = 0; pi < 2; pi++) for (uint32_t k = 0; k < n; k++) {
        const Bytes &proof = *proofs[pi];
        std::unique_ptr<uint8_t[]> blk(new uint8_t[proof.size()]);                 // exactly its own length
        memcpy(blk.get(), proof.data(), proof.size());
        plk_g1_affine hp[25]; plk_fr hs[25]; int32_t early = -1;
        const int32_t rc = verify_terms_parsed(keys[k]->parsed, blk.get(), proof.size(), 0, hp, hs, &early);
        const int want = rc != PLK_OK ? 2 : early;
        VksetKey key;
        EXPECT(vkset_lookup(v, k, &key));
        EXPECT(memcmp(key.front, &keys[k]->front, sizeof(FrontVk)) == 0);
        G1Affine dp[FRONT_PTS]; Fr ds[FRONT_TERMS];
        memset(dp, 0, sizeof dp); memset(ds, 0, sizeof ds);
        const int got = (int)flatten_front(*key.front, blk.get(), blk.get() + proof.size(), dp, ds);
        EXPECT(got == want);
        EXPECT(want == ((pi == 0) == (k != 1) ? 1 : 0));                           // the proof of A goes on under A, is settled under F, and the converse
        if (want == 1 && got == 1) {
            went_on++;
            EXPECT(memcmp(dp, &hp[11], sizeof dp) == 0 && memcmp(ds, hs, sizeof ds) == 0);
            EXPECT(memcmp(key.fixed, hp, 11 * 64) == 0 && memcmp(key.fixed + 11, &hp[22], 64) == 0);   // terms 0..10 and 22 as vm_mul_mixed_kernel takes them
            // and the pairing of the host's two sums over the table the lookup names: left to the GPU tests (the sums are device code)
        } else
            settled++;
    }
    EXPECT(went_on == 3 && settled == 3);
    printf("front: %d (proof, key) pairs go on, %d are settled by the front end\n", went_on, settled);
}

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: verify_mixed_check vkA.bin vkF.bin proofA.bin proofF.bin\n"); return 2; }
    dedup_cases();
    layout_cases();
    index_cases();
    lookup_cases();
    front_cases(slurp(argv[1]), slurp(argv[2]), slurp(argv[3]), slurp(argv[4]));
    printf("%d checks\n", checks);
    printf("%d mismatches\n", bad);
    return bad ? 1 : 0;
}
