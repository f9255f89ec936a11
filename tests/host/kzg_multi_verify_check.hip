// The scalar front of plk_kzg_verify_multi_many_dev (plonkit_amd/csrc/kzg_multi_verify_dev.h: what k_kmv_check runs, one opening per lane)
// compiled for the HOST — its functions are __host__ __device__ — and its plan (kzg_multi_verify_plan.h).  No GPU involved.
// Driver: tests/test_kzg_multi_verify_host.py, which writes the cases and computes every expected number itself.
//
//   kzg_multi_verify_check cases.txt
//
// cases.txt: the number of cases, then per case
//     name  count  npoints  kind  state          kind: the group elements handed over (0 all infinity, 1 all the generator, 2 W' off the
//     the count sets                                   curve, 3 a coordinate of the last commitment = q); state: what the model expects
//     gamma  u  the npoints points  the count x npoints evaluations  the count + 3 expected scalars
// with every field element as the 64 hexadecimal digits of its 256-bit word IN MEMORY (Montgomery; a word >= r is how a non-residue is
// written).  Every array sits in a heap block of exactly its own length, so that the sanitizer build reports a read outside it — an
// evaluation outside a set holds a non-residue in some cases and must not matter.  Each case is held against two references: the expected
// words of the file (the Python-integer model: c_values, r_at, z_at) and km_weights / km_c / km_r_at of kzg_multi_plan.h behind
// plk_kzg_verify_multi's own checks.  It runs twice, with the running products 1 and 3 elements apart.
#include "../../plonkit_amd/csrc/kzg_multi_plan.h"
#include "../../plonkit_amd/csrc/kzg_multi_verify_dev.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace plk;
using namespace plk::host;

static int bad = 0;
static void mismatch(const char *name, const char *what) { bad++; if (bad < 20) printf("MISMATCH %s: %s\n", name, what); }

static Fr read_word(FILE *f) {
    char w[80];
    if (fscanf(f, "%79s", w) != 1 || strlen(w) != 64) { fprintf(stderr, "bad word in the case file\n"); exit(2); }
    Fr v = Fr::zero();
    for (int k = 0; k < 64; k++) {
        const char ch = w[63 - k];
        const uint32_t d = ch <= '9' ? ch - '0' : ch - 'a' + 10;
        v.l[k / 8] |= d << (4 * (k % 8));
    }
    return v;
}
static HFr as_host(const Fr &v) { HFr h; memcpy(h.l, v.l, 32); return h; }
static bool below_r(const Fr &v) { uint64_t w[4]; memcpy(w, v.l, 32); return !HFr::geq_p(w); }

static G1Affine generator() { G1Affine g; g.x = Fq::one(); g.y = add(g.x, g.x); return g; }

// what plk_kzg_verify_multi decides and multiplies by, from kzg_multi_plan.h: false = PLK_ERR_ARG for the opening's own data
static bool by_the_plan_header(uint32_t m, uint32_t p, const uint32_t *sets, const Fr *pts, const Fr *ev, const Fr &gamma, const Fr &u, bool points_ok, HFr *sc) {
    if (!points_ok) return false;
    HFr t[KM_MAX_POINTS];
    for (uint32_t j = 0; j < p; j++) { if (!below_r(pts[j])) return false; t[j] = as_host(pts[j]); }
    if (!below_r(gamma) || !below_r(u)) return false;
    if (km_check_sets(t, p, sets, m) != KM_SETS_OK) return false;
    HFr w[KM_MAX_OPEN * KM_MAX_POINTS], c[KM_MAX_OPEN], z_t, sum = HFr::zero();
    km_weights(t, p, sets, m, w);
    km_c(t, p, sets, m, as_host(gamma), as_host(u), c, &z_t);
    for (uint32_t i = 0; i < m; i++) {
        HFr y[KM_MAX_POINTS];
        for (uint32_t j = 0; j < p; j++) {
            y[j] = HFr::zero();
            if (!((sets[i] >> j) & 1)) continue;
            if (!below_r(ev[i * p + j])) return false;
            y[j] = as_host(ev[i * p + j]);
        }
        sum = sum + c[i] * km_r_at(t, p, sets[i], w + i * p, y, as_host(u));
        sc[i] = c[i];
    }
    sc[m] = -sum; sc[m + 1] = -z_t; sc[m + 2] = as_host(u);
    return true;
}

static uint64_t lane_map(uint64_t n, uint32_t count) {                 // the (opening, term) <-> lane map is a bijection; a checksum of it
    const uint32_t terms = kmv_terms(count);
    const uint64_t lanes = kmv_lanes(n, count);
    std::vector<uint8_t> seen(lanes, 0);
    uint64_t sum = 0;
    for (uint64_t lane = 0; lane < lanes; lane++) {
        const uint32_t o = kmv_lane_opening((uint32_t)lane, count), t = kmv_lane_term((uint32_t)lane, count);
        if (o >= n || t >= terms || kmv_lane(o, t, count) != lane || seen[(size_t)o * terms + t]++) { mismatch("lane map", "not a bijection"); break; }
        if (kmv_term_base(t, count) != (t < count ? 0u : t - count + 1)) mismatch("lane map", "base of a term");
        sum += (lane + 1) * ((uint64_t)o * 64 + t + 1);
    }
    for (uint8_t s : seen) if (s != 1) { mismatch("lane map", "a term without a lane"); break; }
    if (kmv_blocks(lanes) * (uint64_t)KMV_BLOCK < lanes || (kmv_blocks(lanes) - 1) * (uint64_t)KMV_BLOCK >= lanes) mismatch("lane map", "blocks");
    return sum;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: kzg_multi_verify_check cases.txt\n"); return 2; }
    // the plan: the driver holds these lines against its own arithmetic
    const uint32_t shapes[4][2] = {{1, 1}, {3, 2}, {8, 4}, {32, 8}};
    for (const auto &s : shapes) {
        const uint64_t pass = kmv_pass(s[0], s[1]);
        const KmvLayout L = kmv_layout(s[0], s[1], pass);
        printf("plan %u %u terms %u pairs %u bytes %llu pass %llu layout %llu %llu %llu %llu %llu %llu %llu %llu\n", s[0], s[1], kmv_terms(s[0]), kmv_pairs(s[1]),
               (unsigned long long)kmv_bytes_per_opening(s[0], s[1]), (unsigned long long)pass, (unsigned long long)L.scalars, (unsigned long long)L.products,
               (unsigned long long)L.run, (unsigned long long)L.a, (unsigned long long)L.b, (unsigned long long)L.verdict, (unsigned long long)L.state,
               (unsigned long long)L.total);
        if (L.total > KMV_PASS_BYTES || pass % KMV_BLOCK || pass == 0 || pass > KMV_PASS_MAX) mismatch("plan", "a pass outside its limits");
        const KmvLayout odd = kmv_layout(s[0], s[1], 257);
        for (uint64_t off : {odd.scalars, odd.products, odd.run, odd.a, odd.b, odd.verdict, odd.state, odd.total}) if (off % 16) mismatch("plan", "an offset that is not 16-byte aligned");
        if (odd.total < 257 * kmv_bytes_per_opening(s[0], s[1]) || odd.total > 257 * kmv_bytes_per_opening(s[0], s[1]) + 32) mismatch("plan", "padding");
        for (uint64_t n : {1ull, 255ull, 256ull, 257ull}) printf("lanes %llu %u sum %llu\n", (unsigned long long)n, s[0], (unsigned long long)lane_map(n, s[0]));
    }
    for (uint32_t p = 1; p <= KMV_MAX_POINTS; p++) {                   // the pairs in order, without a gap
        uint32_t k = 0;
        for (uint32_t j = 0; j < p; j++) for (uint32_t l = j + 1; l < p; l++, k++) if (kmv_pair(j, l, p) != k) mismatch("plan", "the order of the pairs");
        if (k != kmv_pairs(p)) mismatch("plan", "the number of pairs");
    }

    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int cases = 0, seen[3] = {0, 0, 0};
    if (fscanf(f, "%d", &cases) != 1) { fprintf(stderr, "no case count\n"); return 2; }
    for (int k = 0; k < cases; k++) {
        char name[128];
        unsigned m = 0, p = 0, kind = 0, want = 0;
        if (fscanf(f, "%127s %u %u %u %u", name, &m, &p, &kind, &want) != 5 || m == 0 || m > KMV_MAX_OPEN || p == 0 || p > KMV_MAX_POINTS || kind > 3 || want < 1 || want > 2) {
            fprintf(stderr, "bad case header\n"); return 2; }
        KmvShape S;
        memset(&S, 0, sizeof S);
        S.count = m; S.npoints = p;
        for (unsigned i = 0; i < m; i++) if (fscanf(f, "%u", &S.sets[i]) != 1) return 2;
        const uint32_t terms = kmv_terms(m), pairs = kmv_pairs(p);
        std::unique_ptr<Fr[]> gamma(new Fr[1]), u(new Fr[1]), pts(new Fr[p]), ev(new Fr[m * p]), expect(new Fr[terms]);
        std::unique_ptr<G1Affine[]> cm(new G1Affine[m]), proofs(new G1Affine[2]);
        gamma[0] = read_word(f); u[0] = read_word(f);
        for (unsigned j = 0; j < p; j++) pts[j] = read_word(f);
        for (unsigned j = 0; j < m * p; j++) ev[j] = read_word(f);
        for (unsigned t = 0; t < terms; t++) expect[t] = read_word(f);
        memset(cm.get(), 0, m * sizeof(G1Affine)); memset(proofs.get(), 0, 2 * sizeof(G1Affine));
        if (kind) { for (unsigned i = 0; i < m; i++) cm[i] = generator(); proofs[0] = generator(); proofs[1] = generator(); }
        if (kind == 2) proofs[1].y = add(proofs[1].y, Fq::one());      // (1, 3)
        if (kind == 3) memcpy(cm[m - 1].x.l, FqParams::P, 32);
        std::vector<HFr> plan(terms, HFr::zero());
        const bool plan_ok = by_the_plan_header(m, p, S.sets, pts.get(), ev.get(), gamma[0], u[0], kind < 2, plan.data());
        if (!plan_ok) plan.assign(terms, HFr::zero());                 // a refusal half-way leaves nothing behind
        for (size_t stride : {(size_t)1, (size_t)3}) {
            std::unique_ptr<Fr[]> run(new Fr[pairs * stride]), sc(new Fr[terms]);
            memset(run.get(), 0xA5, pairs * stride * sizeof(Fr)); memset(sc.get(), 0xA5, terms * sizeof(Fr));
            const uint32_t got = kmv_front(S, cm.get(), pts.get(), ev.get(), gamma.get(), u.get(), proofs.get(), run.get(), stride, sc.get());
            if (got != want) mismatch(name, "the state is not the model's");
            if (got != (plan_ok ? KMV_STATE_GOES_ON : KMV_STATE_MALFORMED)) mismatch(name, "the state is not plk_kzg_verify_multi's");
            if (memcmp(sc.get(), expect.get(), terms * sizeof(Fr)) != 0) mismatch(name, "the scalars are not the model's");
            if (memcmp(sc.get(), plan.data(), terms * sizeof(Fr)) != 0) mismatch(name, "the scalars are not kzg_multi_plan.h's");
            if (stride == 3) for (size_t e = 0; e < (size_t)pairs * 3; e++) if (e % 3) { Fr a5; memset(&a5, 0xA5, sizeof a5); if (!(run[e] == a5)) { mismatch(name, "a write between the slots"); break; } }
        }
        seen[want]++;
    }
    fclose(f);
    printf("kzg_multi_verify_check: %d cases, %d go on, %d malformed, %d mismatches\n", cases, seen[1], seen[2], bad);
    return bad ? 1 : 0;
}
