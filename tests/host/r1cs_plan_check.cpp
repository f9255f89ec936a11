// Stand-alone check of plonkit_amd/csrc/r1cs_plan.h (the host half of the R1CS witness check): hand-made R1CS structures go
// through r1cs_plan_build, and the plan is compared with its source term by term and, evaluated with hostmath.h, with a direct
// loop over R1cs::lc.  Built with -fsanitize=address,undefined by tests/test_r1cs_plan_host.py and run directly.
#include "../../plonkit_amd/csrc/r1cs_plan.h"
#include <cstdio>
#include <cstdlib>

using namespace plk;

// circuit.h declares it; the library defines it in hostapi.cpp, which this program does not link
void plk::set_error(const std::string &) {}

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static HFr rnd_fr() { uint64_t c[4] = {rnd(), rnd(), rnd(), rnd() >> 3}; return HFr::from_canonical(c); }   // < 2^253 < r

static int failures = 0, cases = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: %s — ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// the reference verdict: a direct loop over R1cs::lc, wire 0 read as 1
static HFr direct_lc(const R1cs &r, size_t i, int which, const std::vector<HFr> &w) {
    HFr acc = HFr::zero();
    for (const LcTerm &t : r.lc(i, which)) acc = acc + t.coeff * (t.wire == 0 ? HFr::one() : w[t.wire]);
    return acc;
}
static uint64_t direct_check(const R1cs &r, const std::vector<HFr> &w) {
    for (size_t i = 0; i < r.num_constraints(); i++)
        if (direct_lc(r, i, 0, w) * direct_lc(r, i, 1, w) != direct_lc(r, i, 2, w)) return i;
    return ~0ull;
}

static void check_plan(const char *name, const R1cs &r, const std::vector<std::vector<HFr>> &witnesses, const std::vector<uint64_t> &expect_bad,
                       size_t expect_table = 0) {
    cases++;
    R1csPlan p;
    std::string err;
    const uint32_t L = R1CS_LONG_LC_TERMS;
    EXPECT(r1cs_plan_build(r, &p, &err), "%s: build refused: %s", name, err.c_str());
    const size_t m = r.num_constraints();
    EXPECT(p.num_constraints == m && p.num_variables == r.num_variables, "%s: sizes", name);
    EXPECT(p.terms.size() == r.terms.size() && p.off.size() == 3 * m + 1, "%s: lengths", name);
    EXPECT(p.table.size() >= 2 && p.table[0] == HFr::one() && p.table[1] == HFr::zero() - HFr::one(), "%s: table[0], table[1]", name);
    if (expect_table) EXPECT(p.table.size() == expect_table, "%s: table has %zu entries, expected %zu", name, p.table.size(), expect_table);
    for (size_t a = 0; a < p.table.size(); a++)
        for (size_t b = a + 1; b < p.table.size() && p.table.size() <= 512; b++) EXPECT(p.table[a] != p.table[b], "%s: table entries %zu and %zu are equal", name, a, b);
    for (size_t k = 0; k < p.terms.size() && k < r.terms.size(); k++) {
        EXPECT(p.terms[k].coeff < p.table.size(), "%s: term %zu: index beyond the table", name, k);
        if (p.terms[k].coeff < p.table.size())
            EXPECT(p.terms[k].wire == r.terms[k].wire && p.table[p.terms[k].coeff] == r.terms[k].coeff, "%s: term %zu differs from its source", name, k);
    }
    for (size_t j = 0; j + 1 < p.off.size(); j++) EXPECT(p.off[j] <= p.off[j + 1] && p.off[j] == r.off[j], "%s: offset %zu", name, j);
    EXPECT(p.off.empty() || p.off.back() == p.terms.size(), "%s: last offset", name);
    std::vector<int> seen(3 * m, 0);
    for (size_t k = 0; k < p.short_lcs.size(); k++) {
        const uint32_t j = p.short_lcs[k];
        EXPECT(j < 3 * m, "%s: short list entry", name);
        if (j >= 3 * m) continue;
        seen[j]++;
        EXPECT(p.off[j + 1] - p.off[j] < L, "%s: LC %u of %llu terms in the short list", name, j, (unsigned long long)(p.off[j + 1] - p.off[j]));
        if (k) EXPECT(p.short_lcs[k - 1] < j, "%s: the short list is not in LC order", name);
    }
    for (uint32_t j : p.long_lcs) {
        EXPECT(j < 3 * m, "%s: long list entry", name);
        if (j >= 3 * m) continue;
        seen[j]++;
        EXPECT(p.off[j + 1] - p.off[j] >= L, "%s: LC %u of %llu terms in the long list", name, j, (unsigned long long)(p.off[j + 1] - p.off[j]));
    }
    for (size_t j = 0; j < 3 * m; j++) EXPECT(seen[j] == 1, "%s: LC %zu is in %d work lists", name, j, seen[j]);
    for (size_t k = 0; k < witnesses.size(); k++) {
        const uint64_t direct = direct_check(r, witnesses[k]), plan = r1cs_plan_check_host(p, witnesses[k].data());
        EXPECT(direct == plan, "%s: witness %zu: direct loop says %llu, the plan %llu", name, k, (unsigned long long)direct, (unsigned long long)plan);
        if (k < expect_bad.size()) EXPECT(plan == expect_bad[k], "%s: witness %zu: expected %llu, got %llu", name, k, (unsigned long long)expect_bad[k], (unsigned long long)plan);
    }
}

enum CoeffKind { ALL_DISTINCT, ALL_EQUAL, PLUS_MINUS_ONE, MIXED };
static HFr pick_coeff(CoeffKind kind, const HFr &equal) {
    switch (kind) {
    case ALL_DISTINCT: return rnd_fr();
    case ALL_EQUAL: return equal;
    case PLUS_MINUS_ONE: return (rnd() & 1) ? HFr::one() : HFr::zero() - HFr::one();
    default: { const uint64_t s = rnd() % 4; return s == 0 ? HFr::one() : (s == 1 ? HFr::zero() - HFr::one() : (s == 2 ? HFr::from_u64(2) : rnd_fr())); }
    }
}

// m constraints; A and B of the given lengths over random earlier wires (wire 0 and repeated wires included), C closed through a
// fresh wire so that the returned witness satisfies every constraint: C = (c_len - 1 random terms) + 1 * fresh
static void build_chain(size_t m, const std::vector<size_t> &lens, CoeffKind kind, R1cs *r, std::vector<HFr> *w) {
    const HFr equal = rnd_fr();
    const size_t base = 8;
    r->clear();
    r->num_inputs = 2; r->num_variables = base + m; r->num_aux = r->num_variables - r->num_inputs;
    w->assign(r->num_variables, HFr::zero());
    (*w)[0] = HFr::one();
    for (size_t v = 1; v < base; v++) (*w)[v] = v == 1 ? HFr::zero() : (v == 2 ? HFr::zero() - HFr::one() : rnd_fr());
    size_t pick = 0;
    for (size_t i = 0; i < m; i++) {
        HFr val[3];
        for (int which = 0; which < 3; which++) {
            const size_t len = lens[pick++ % lens.size()];
            Lc lc;
            HFr acc = HFr::zero();
            const size_t free_terms = which == 2 && len ? len - 1 : len;
            for (size_t k = 0; k < free_terms; k++) {
                const uint32_t wire = (uint32_t)(rnd() % (base + i));
                const HFr c = pick_coeff(kind, equal);
                lc.push_back(LcTerm{wire, c});
                acc = acc + c * (wire == 0 ? HFr::one() : (*w)[wire]);
            }
            val[which] = acc;
            if (which == 2 && len) {                             // close C: coefficient c on the fresh wire, value (a * b - acc) / c
                const HFr c = kind == ALL_DISTINCT ? rnd_fr() : (kind == ALL_EQUAL ? equal : HFr::one());
                lc.push_back(LcTerm{(uint32_t)(base + i), c});
                (*w)[base + i] = (val[0] * val[1] - acc) * c.inv();
            }
            r->push_lc(lc.data(), lc.size());
        }
        // (an empty C is only satisfied when a * b = 0: the callers give empty C an empty A or B)
    }
}

int main() {
    const size_t L = R1CS_LONG_LC_TERMS;

    {   // no constraints at all
        R1cs r; r.num_inputs = 1; r.num_variables = 1;
        check_plan("empty", r, {{HFr::one()}}, {~0ull}, 2);
    }
    {   // one constraint: w1 * w1 = w2
        R1cs r; r.num_inputs = 1; r.num_variables = 3; r.num_aux = 2;
        LcTerm a{1, HFr::one()}, c{2, HFr::one()};
        r.push_lc(&a, 1); r.push_lc(&a, 1); r.push_lc(&c, 1);
        const HFr x = rnd_fr();
        check_plan("one constraint", r, {{HFr::one(), x, x * x}, {HFr::one(), x, x * x + HFr::one()}, {HFr::zero(), x, x * x}, {rnd_fr(), x, x * x}},
                   {~0ull, 0, ~0ull, ~0ull}, 2);
    }
    {   // empty LCs: 0 * B = 0 and A * 0 = 0 hold by arithmetic; (empty) * B = C does not unless C evaluates to 0
        R1cs r; r.num_inputs = 1; r.num_variables = 3; r.num_aux = 2;
        LcTerm t1{1, HFr::from_u64(3)}, t2{2, HFr::one()};
        r.push_lc(nullptr, 0); r.push_lc(&t1, 1); r.push_lc(nullptr, 0);
        r.push_lc(&t1, 1); r.push_lc(nullptr, 0); r.push_lc(nullptr, 0);
        r.push_lc(nullptr, 0); r.push_lc(nullptr, 0); r.push_lc(nullptr, 0);
        r.push_lc(nullptr, 0); r.push_lc(&t1, 1); r.push_lc(&t2, 1);
        check_plan("empty LCs", r, {{HFr::one(), rnd_fr(), HFr::zero()}, {HFr::one(), rnd_fr(), HFr::one()}}, {~0ull, 3}, 3);
    }
    {   // wire 0 with a coefficient, the same wire twice: (2 * one + w1 + w1) * (one) = w2
        R1cs r; r.num_inputs = 1; r.num_variables = 3; r.num_aux = 2;
        LcTerm a[3] = {{0, HFr::from_u64(2)}, {1, HFr::one()}, {1, HFr::one()}}, b{0, HFr::one()}, c{2, HFr::one()};
        r.push_lc(a, 3); r.push_lc(&b, 1); r.push_lc(&c, 1);
        const HFr x = rnd_fr(), y = HFr::from_u64(2) + x + x;
        check_plan("wire 0", r, {{HFr::one(), x, y}, {HFr::zero(), x, y}, {rnd_fr(), x, y}, {HFr::one(), x, y + HFr::one()}}, {~0ull, ~0ull, ~0ull, 0}, 3);
    }
    // LC lengths around the threshold and beyond, every kind of coefficient population
    const std::vector<size_t> lens = {1, 2, 3, L - 1, L, L + 1, 63, 64, 65, 129, 5, 1, 1, 2};   // (14 lengths, 3 per constraint: every length meets every side)
    const CoeffKind kinds[4] = {ALL_DISTINCT, ALL_EQUAL, PLUS_MINUS_ONE, MIXED};
    const char *kind_names[4] = {"all distinct", "all equal", "only +-1", "mixed"};
    for (int k = 0; k < 4; k++) {
        R1cs r;
        std::vector<HFr> w;
        const size_t m = 70;
        build_chain(m, lens, kinds[k], &r, &w);
        std::vector<std::vector<HFr>> ws = {w};
        std::vector<uint64_t> expect = {~0ull};
        for (size_t broken : {(size_t)0, (size_t)17, m - 1}) {           // the fresh wire of constraint `broken` is read by its C first
            std::vector<HFr> v = w;
            v[8 + broken] = v[8 + broken] + HFr::one();
            ws.push_back(v);
        }
        {   // two wires broken: the verdict is the lower constraint (a later constraint may read the wire too, never an earlier one)
            std::vector<HFr> v = w;
            v[8 + 40] = v[8 + 40] + HFr::one(); v[8 + 9] = v[8 + 9] + HFr::one();
            ws.push_back(v);
        }
        { std::vector<HFr> v = w; v[0] = HFr::zero(); ws.push_back(v); expect.resize(5, 0); expect[1] = 0; expect[2] = 17; expect[3] = m - 1; expect[4] = 9; expect.push_back(~0ull); }
        size_t expect_table = 0;
        if (kinds[k] == ALL_EQUAL) expect_table = 3;
        if (kinds[k] == PLUS_MINUS_ONE) expect_table = 2;
        if (kinds[k] == ALL_DISTINCT) expect_table = 2 + r.terms.size();   // as long as the term list (random 253-bit values do not collide)
        check_plan(kind_names[k], r, ws, expect, expect_table);
    }
    {   // refusals: a wire beyond num_variables
        R1cs r; r.num_inputs = 1; r.num_variables = 2; r.num_aux = 1;
        LcTerm a{2, HFr::one()};
        r.push_lc(&a, 1); r.push_lc(&a, 1); r.push_lc(&a, 1);
        R1csPlan p; std::string err;
        cases++;
        EXPECT(!r1cs_plan_build(r, &p, &err) && !err.empty(), "a term on wire num_variables was accepted");
    }
    if (failures) { fprintf(stderr, "r1cs_plan_check: %d failures\n", failures); return 1; }
    printf("r1cs_plan_check: ok, %d cases, long = %zu\n", cases, L);
    return 0;
}
