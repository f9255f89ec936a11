// The device front end of the verifier (plonkit_amd/csrc/verify_front_dev.h: Keccak, the rolling transcript, the byte parser, the flattening)
// compiled for the HOST — its functions are __host__ __device__ — against the host code it restates: keccak256, RollingKeccak and
// verify_terms_parsed (parse_proof + flatten_keccak).  Every proof is handed over in a heap block of exactly its own length, so that the
// sanitizer build of this same program reports a read past the end.  No GPU involved.  Driver: tests/test_verify_front_host.py.
//
//   verify_front_check vk.bin proof.bin [list]      list: lines "<vk file> <proof file> <flags>" of further cases made by the driver
#include "../../plonkit_amd/csrc/hostapi.cpp"
#include "../../plonkit_amd/csrc/pairing.cpp"
#include "../../plonkit_amd/csrc/verify.cpp"
#include "../../plonkit_amd/csrc/verify_front_dev.h"
#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>

namespace plk {
static thread_local std::string g_err;
void set_error(const std::string &m) { g_err = m; }
}
extern "C" const char *plk_last_error(void) { return plk::g_err.c_str(); }

typedef std::vector<uint8_t> Bytes;
static Bytes slurp(const std::string &p) { std::ifstream f(p, std::ios::binary); return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;                  // xorshift64*: a fixed seed, the same cases on every run
static uint64_t rnd() { rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27; return rng_state * 0x2545f4914f6cdd1dULL; }

static const uint8_t R_BE[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                                 0x28, 0x33, 0xe8, 0x48, 0x79, 0xb9, 0x70, 0x91, 0x43, 0xe1, 0xf5, 0x93, 0xf0, 0x00, 0x00, 0x01};
static const uint8_t Q_BE[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                                 0x97, 0x81, 0x6a, 0x91, 0x68, 0x71, 0xca, 0x8d, 0x3c, 0x20, 0x8c, 0x16, 0xd8, 0x7c, 0xfd, 0x47};

static int bad = 0;
static int seen[3] = {0, 0, 0};                                       // the host's states over everything compared

struct Key {
    plk::ParsedVk *parsed = nullptr;
    plk::FrontVk front;
    Key(const Bytes &vk, uint32_t flags) {
        parsed = plk::parsed_vk_new(vk.data(), vk.size());
        if (!parsed) { fprintf(stderr, "verification key does not parse\n"); exit(2); }
        plk_fr nr[3], om;
        memset(&front, 0, sizeof front);
        plk::parsed_vk_front(parsed, &front.n, &front.num_inputs, nr, &om);
        front.flags = flags;
        memcpy(front.non_residues, nr, sizeof nr); memcpy(&front.omega, &om, 32);
    }
    ~Key() { plk::parsed_vk_free(parsed); }
};

// the state of both, and for state 1 the 11 points and the 25 scalars word for word; returns the host's state
static int compare(const Key &key, const Bytes &proof, const char *what, long k = -1) {
    std::unique_ptr<uint8_t[]> blk(new uint8_t[proof.size()]);        // exactly its own length, and not null at length 0
    if (!proof.empty()) memcpy(blk.get(), proof.data(), proof.size());
    plk_g1_affine hp[25]; plk_fr hs[25]; int32_t early = -1;
    const int32_t rc = plk::verify_terms_parsed(key.parsed, blk.get(), proof.size(), key.front.flags, hp, hs, &early);
    const int want = rc != PLK_OK ? 2 : early;
    plk::G1Affine dp[plk::FRONT_PTS]; plk::Fr ds[plk::FRONT_TERMS];
    memset(dp, 0, sizeof dp); memset(ds, 0, sizeof ds);
    const int got = (int)plk::flatten_front(key.front, blk.get(), blk.get() + proof.size(), dp, ds);
    seen[want]++;
    bool same = want == got;
    if (same && want == 1) same = memcmp(dp, &hp[11], sizeof dp) == 0 && memcmp(ds, hs, sizeof ds) == 0 && memcmp(&dp[9], &hp[23], 128) == 0;
    if (!same) { bad++; if (bad < 20) printf("MISMATCH %s %ld: host state %d, device-code state %d%s\n", what, k, want, got, want == got ? " (terms differ)" : ""); }
    return want;
}

static void put_u64(Bytes &b, size_t at, uint64_t v) { for (int i = 0; i < 8; i++) b[at + i] = (uint8_t)(v >> (8 * (7 - i))); }
static uint64_t get_u64(const Bytes &b, size_t at) { uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | b[at + i]; return v; }

// byte offsets of a well-formed proof with ni inputs
struct Layout {
    size_t n, cnt_in, in, cnt_w, w, gp, cnt_q, q, cnt_wz, wz, cnt_wzw, wzw, z_zw, t_z, r_z, cnt_sz, sz, oz, ozw, end;
    explicit Layout(size_t ni) {
        size_t o = 0;
        n = o; o += 8; cnt_in = o; o += 8; in = o; o += 32 * ni; cnt_w = o; o += 8; w = o; o += 256; gp = o; o += 64; cnt_q = o; o += 8; q = o; o += 256;
        cnt_wz = o; o += 8; wz = o; o += 128; cnt_wzw = o; o += 8; wzw = o; o += 32; z_zw = o; o += 32; t_z = o; o += 32; r_z = o; o += 32;
        cnt_sz = o; o += 8; sz = o; o += 96; oz = o; o += 64; ozw = o; o += 64; end = o;
    }
    std::vector<size_t> boundaries(size_t ni) const {
        std::vector<size_t> b = {n, cnt_in};
        for (size_t i = 0; i <= ni; i++) b.push_back(in + 32 * i);
        for (size_t base : {w, q}) for (int j = 0; j <= 4; j++) { b.push_back(base + 64 * j); b.push_back(base + 64 * j + 32); }
        b.insert(b.end(), {gp, gp + 32, cnt_q, cnt_wz, wz, wz + 32, wz + 64, wz + 96, cnt_wzw, wzw, z_zw, t_z, r_z, cnt_sz, sz, sz + 32, sz + 64, oz, oz + 32, ozw, ozw + 32, end});
        return b;
    }
    std::vector<size_t> points() const { std::vector<size_t> p; for (int j = 0; j < 4; j++) p.push_back(w + 64 * j); p.push_back(gp); for (int j = 0; j < 4; j++) p.push_back(q + 64 * j); p.push_back(oz); p.push_back(ozw); return p; }
    std::vector<size_t> scalars(size_t ni) const {
        std::vector<size_t> s; for (size_t i = 0; i < ni; i++) s.push_back(in + 32 * i);
        for (int j = 0; j < 4; j++) s.push_back(wz + 32 * j);
        s.insert(s.end(), {wzw, z_zw, t_z, r_z, sz, sz + 32, sz + 64});
        return s;
    }
    std::vector<size_t> counts() const { return {cnt_in, cnt_w, cnt_q, cnt_wz, cnt_wzw, cnt_sz}; }
};

static void random_below_r(uint8_t out[32]) { for (int i = 0; i < 32; i++) out[i] = (uint8_t)rnd(); out[0] &= 0x1f; }

// ---------------------------------------------------------------------------------------------- Keccak and the transcript
static void keccak_cases() {
    for (uint32_t len = 0; len <= 135; len++) {
        uint8_t msg[136] = {0}, want[32];
        for (uint32_t i = 0; i < len; i++) msg[i] = (uint8_t)rnd();
        plk::keccak256(msg, len, want);
        uint64_t lanes[17], got[4];
        memcpy(lanes, msg, 136);
        plk::keccak256_one_block(lanes, len, got);
        if (memcmp(got, want, 32) != 0) { bad++; printf("MISMATCH keccak256 at length %u\n", len); }
    }
    for (int seq = 0; seq < 300; seq++) {
        plk::RollingKeccak h; plk::RollingKeccakDev d; plk::rk_init(d);
        const int steps = 1 + (int)(rnd() % 24);
        for (int s = 0; s < steps; s++) {
            const uint64_t kind = rnd() % 3;
            uint8_t b[32];
            if (kind == 0) {
                random_below_r(b);
                plk::host::HFr x; plk::host::HFr::from_be_bytes(b, &x);
                plk::Fr y; memcpy(y.l, x.l, 32);
                h.absorb_fr(x); plk::rk_absorb_fr(d, y);
            } else if (kind == 1) {                                   // any two coordinates: the transcript does not look at the curve
                plk::host::HAffine p; plk::G1Affine q;
                random_below_r(b); plk::host::HFq::from_be_bytes(b, &p.x);
                random_below_r(b); plk::host::HFq::from_be_bytes(b, &p.y);
                if (rnd() % 8 == 0) { p.x = plk::host::HFq::zero(); p.y = plk::host::HFq::zero(); }
                memcpy(q.x.l, p.x.l, 32); memcpy(q.y.l, p.y.l, 32);
                h.absorb_g1(p); plk::rk_absorb_g1(d, q);
            } else {
                const plk::host::HFr x = h.challenge(); const plk::Fr y = plk::rk_challenge(d);
                if (memcmp(x.l, y.l, 32) != 0) { bad++; printf("MISMATCH transcript %d: challenge at step %d\n", seq, s); break; }
            }
            if (memcmp(h.s0, d.s, 32) != 0 || memcmp(h.s1, d.s + 4, 32) != 0 || h.counter != d.counter) { bad++; printf("MISMATCH transcript %d: state at step %d\n", seq, s); break; }
        }
    }
}

// ---------------------------------------------------------------------------------------------- built-in proofs
static void structural_cases(const Bytes &vk, const Bytes &proof) {
    const Key key(vk, 0);
    const size_t ni = (size_t)get_u64(proof, 8);
    const Layout L(ni);
    if (L.end != proof.size()) { fprintf(stderr, "the golden proof has not the expected layout\n"); exit(2); }
    if (compare(key, proof, "golden") != 1) { bad++; printf("golden: the host does not go on\n"); }
    // cut at every field boundary and one byte either side of it; a trailing byte
    for (size_t b : L.boundaries(ni)) for (long d = -1; d <= 1; d++) {
        const long len = (long)b + d;
        if (len < 0 || len >= (long)proof.size()) continue;
        if (compare(key, Bytes(proof.begin(), proof.begin() + len), "cut", len) != 2) { bad++; printf("cut %ld: host state\n", len); }
    }
    { Bytes t = proof; t.push_back(0); if (compare(key, t, "trailing byte") != 2) { bad++; printf("trailing byte: host state\n"); } }
    compare(key, Bytes(), "empty");
    // each count field at +-1 and 2^61 (2^61 * 32 wraps to 0 in 64 bits: only the division keeps the bound)
    for (size_t c : L.counts()) {
        const uint64_t v = get_u64(proof, c);
        for (uint64_t nv : {v + 1, v - 1, (uint64_t)1 << 61, ~(uint64_t)0}) { Bytes t = proof; put_u64(t, c, nv); compare(key, t, "count", (long)c); }
    }
    {   // the input count moved WITH its bytes: a well-formed proof of another input count is a verdict, not malformed
        Bytes more(proof.begin(), proof.begin() + L.in + 32 * ni); put_u64(more, 8, ni + 1); more.insert(more.end(), 32, 0); more.insert(more.end(), proof.begin() + L.cnt_w, proof.end());
        if (compare(key, more, "one more input") != 0) { bad++; printf("one more input: host state\n"); }
        if (ni) {
            Bytes less(proof.begin(), proof.begin() + L.in + 32 * (ni - 1)); put_u64(less, 8, ni - 1); less.insert(less.end(), proof.begin() + L.cnt_w, proof.end());
            if (compare(key, less, "one input less") != 0) { bad++; printf("one input less: host state\n"); }
        }
        Bytes t = proof; put_u64(t, 0, get_u64(proof, 0) + 8);          // another n
        if (compare(key, t, "another n in the proof") != 0) { bad++; printf("another n: host state\n"); }
    }
    // a coordinate equal to q (and q - 1: off the curve or not, both must agree), a scalar equal to r (and r - 1: a verdict)
    for (size_t p : L.points()) for (int half = 0; half < 2; half++) for (int minus = 0; minus < 2; minus++) {
        Bytes t = proof; memcpy(&t[p + 32 * half], Q_BE, 32); t[p + 32 * half + 31] -= (uint8_t)minus;
        const int s = compare(key, t, "coordinate q", (long)p);
        if (!minus && s != 2) { bad++; printf("coordinate = q at %zu: host state %d\n", p, s); }
    }
    for (size_t sc : L.scalars(ni)) for (int minus = 0; minus < 2; minus++) {
        Bytes t = proof; memcpy(&t[sc], R_BE, 32); t[sc + 31] -= (uint8_t)minus;
        const int s = compare(key, t, "scalar r", (long)sc);
        if ((minus ? s == 2 : s != 2)) { bad++; printf("scalar = r - %d at %zu: host state %d\n", minus, sc, s); }
    }
    // flags: 0x80, 0x40 on a live point, both; the infinity encoding (a verdict), and with a non-zero tail at every byte
    for (size_t p : L.points()) {
        for (uint8_t f : {0x80, 0x40, 0xc0}) { Bytes t = proof; t[p] |= f; if (compare(key, t, "flag", (long)p) != 2 && t[p] != proof[p]) { bad++; printf("flag %x at %zu: host state\n", f, p); } }
        Bytes inf = proof; memset(&inf[p], 0, 64); inf[p] = 0x40;
        if (compare(key, inf, "infinity", (long)p) == 2) { bad++; printf("infinity at %zu: host state\n", p); }
        for (int at : {1, 31, 32, 63}) { Bytes t = inf; t[p + at] = 1; if (compare(key, t, "infinity with a tail", (long)p) != 2) { bad++; printf("infinity tail: host state\n"); } }
        Bytes both = inf; both[p] = 0xc0; compare(key, both, "both flags, zero tail", (long)p);
        Bytes zero = proof; memset(&zero[p], 0, 64);                  // (0, 0) unflagged
        if (compare(key, zero, "unflagged zero", (long)p) != 2) { bad++; printf("unflagged (0, 0): host state\n"); }
    }
    // wrong keys: another n (a domain and none), another input count, the strict rule on a zero-input key
    for (uint64_t n : {(uint64_t)15, (uint64_t)8, (uint64_t)0, ~(uint64_t)0, ((uint64_t)1 << 29) - 1}) { Bytes k2 = vk; put_u64(k2, 0, n); compare(Key(k2, 0), proof, "key of another n"); }
    for (uint64_t c : {(uint64_t)0, (uint64_t)2, (uint64_t)40}) { Bytes k2 = vk; put_u64(k2, 8, c); compare(Key(k2, 0), proof, "key of another input count"); compare(Key(k2, 1), proof, "the same, strict"); }
    {
        Bytes k0 = vk; put_u64(k0, 8, 0);
        Bytes p0(proof.begin(), proof.begin() + L.in); put_u64(p0, 8, 0); p0.insert(p0.end(), proof.begin() + L.cnt_w, proof.end());
        compare(Key(k0, 0), p0, "zero-input key");
        if (compare(Key(k0, 1), p0, "zero-input key, strict") != 0) { bad++; printf("strict rule: host state\n"); }
        compare(Key(vk, 1), proof, "strict, one input");
    }
}

// ---------------------------------------------------------------------------------------------- the byte-mutation run
// Three kinds in equal parts, chosen so that the HOST puts at least a tenth of the cases into each state (asserted on the host's answers):
//   goes on   what the equation at z does not see: d(z omega), an opening proof replaced by another point of the proof or negated
//   invalid   a scalar of the equation replaced by a random one, a commitment the transcript absorbs replaced by another point, another n
//   anything  1..3 random bytes set to random values, or a random cut (mostly malformed: a random x is seldom on the curve)
static void fuzz(const Bytes &vk, const Bytes &proof, int cases) {
    const Key key(vk, 0);
    const size_t ni = (size_t)get_u64(proof, 8);
    const Layout L(ni);
    const std::vector<size_t> pts = L.points(), scs = L.scalars(ni);
    int st[3] = {0, 0, 0};
    for (int k = 0; k < cases; k++) {
        Bytes t = proof;
        const uint64_t kind = rnd() % 3, pick = rnd();
        if (kind == 0) {
            if (pick % 4 == 0) random_below_r(&t[L.wzw]);
            else if (pick % 4 == 1) memcpy(&t[pick & 8 ? L.oz : L.ozw], &proof[pts[(pick >> 8) % pts.size()]], 64);
            else if (pick % 4 == 2) { memcpy(&t[L.oz], &proof[L.ozw], 64); memcpy(&t[L.ozw], &proof[L.oz], 64); }
            else { memset(&t[pick & 8 ? L.oz : L.ozw], 0, 64); t[pick & 8 ? L.oz : L.ozw] = 0x40; random_below_r(&t[L.wzw]); }
        } else if (kind == 1) {
            if (pick % 3 == 0) { size_t s; do s = scs[(rnd() >> 8) % scs.size()]; while (s == L.wzw); random_below_r(&t[s]); }
            else if (pick % 3 == 1) { const size_t dst = pts[(pick >> 8) % 9], src = pts[(pick >> 16) % pts.size()]; if (dst == src) t[L.t_z + 31] ^= 1; else memcpy(&t[dst], &proof[src], 64); }
            else put_u64(t, 0, (pick >> 8) % 3 ? rnd() : 15);
        } else {
            if (pick % 5 == 0) t.resize((pick >> 8) % (proof.size() + 1));
            else for (uint64_t j = 0; j <= (pick >> 8) % 3; j++) t[rnd() % t.size()] = (uint8_t)rnd();
        }
        st[compare(key, t, "fuzz", k)]++;
    }
    printf("fuzz: %d cases, host states: %d invalid, %d go on, %d malformed\n", cases, st[0], st[1], st[2]);
    for (int s = 0; s < 3; s++) if (st[s] * 10 < cases) { bad++; printf("fuzz: fewer than a tenth of the cases in host state %d\n", s); }
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: verify_front_check vk.bin proof.bin [list]\n"); return 2; }
    const Bytes vk = slurp(argv[1]), proof = slurp(argv[2]);
    keccak_cases();
    structural_cases(vk, proof);
    int listed = 0;
    if (argc > 3) {
        std::ifstream f(argv[3]);
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream is(line);
            std::string vkf, pf; uint32_t flags = 0;
            if (!(is >> vkf >> pf >> flags)) continue;
            compare(Key(slurp(vkf), flags), slurp(pf), pf.c_str());
            listed++;
        }
    }
    fuzz(vk, proof, 3000);
    printf("%d listed cases; host states over all comparisons: %d invalid, %d go on, %d malformed\n", listed, seen[0], seen[1], seen[2]);
    printf("%d mismatches\n", bad);
    return bad ? 1 : 0;
}
