// Host-side check of the products with a folded addend (field29_dev.h: mulw2_add) and of the mixed addition built on them
// (ec29_dev.h: xyzzw_add_mixed_flag, the addition of msm_accumulate's plain kernel) against the forms they replace.
// Built and run by tests/test_field29_addend_host.py with hipcc; needs no GPU.  A stand-alone program: it may also be built with
// -Xarch_host -fsanitize=address,undefined and run directly.
//   1. mulw2_add(a, b, A) == mulw(a, b) followed by the padded addition and normw, bit for bit: random operands, and operands at the
//      documented bounds (left operand limbs at MULW_A_LIMB_MAX, addend limbs at 2^32 - 1, accumulator coordinates at 6p / 1.3p);
//      a 128-bit shadow of the column chain shows that the 64-bit accumulator never overflows there.
//   2. mul2addw with the un-normalised Q - X3 + 6p and 2p - PPP (pads with a 2^29 bias) as right operands == the same with the
//      normalised sub6 / neg2, bit for bit; the pads are 6p and 2p; the column bound at the limb bounds (128-bit shadow).
//   3. xyzzw_add_mixed_flag against a reference copy of xyzzw_add_mixed as it was before the addends were folded: > 10^5 random and
//      edge operands (P = +-Q, accumulator at the identity, y negated, coordinates at their bounds): bit for bit where y is not
//      negated, as residues mod p where it is (the sign now goes onto the affine operand, so R differs by a multiple of p).
#include "ec29_dev.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace plk;
typedef unsigned __int128 u128;
static uint64_t rs = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 16); }
static Fq rnd_fq() { Fq a; for (int i = 0; i < 8; i++) a.l[i] = rnd(); a.l[7] &= 0x0fffffff; return a; }   // < 2^252 < p
static FqW9 rnd_w() { return w_from_s(unpack<FqW>(rnd_fq())); }                                          // < 1.1p, normalised
static bool same(const FqW9 &a, const FqW9 &b) { for (int i = 0; i < 9; i++) if (a.l[i] != b.l[i]) return false; return true; }
static bool less(const FqW9 &a, const FqW9 &b) { for (int i = 8; i >= 0; i--) if (a.l[i] != b.l[i]) return a.l[i] < b.l[i]; return false; }
// num * p / den, normalised
static FqW9 p_times(uint32_t num, uint32_t den = 1) {
    uint64_t t[9], c = 0;
    for (int i = 0; i < 9; i++) { c += (uint64_t)num * FqW::P29[i]; t[i] = c & M29; c >>= 29; }
    t[8] += c << 29;
    FqW9 r; uint64_t rem = 0;
    for (int i = 8; i >= 0; i--) { const uint64_t v = (rem << 29) + t[i]; r.l[i] = (uint32_t)(v / den); rem = v % den; }
    return r;
}
static FqW9 minus_one(FqW9 a) { int i = 0; while (a.l[i] == 0) { a.l[i] = M29; i++; } a.l[i]--; return a; }
// the forms that were replaced: product, then limb-wise addition of the addend, then carry propagation (64-bit, so that addend limbs
// up to 2^32 - 1 can be checked; equal to normw(addw(.)) wherever that is defined, which is checked too)
static FqW9 add_norm64(const FqW9 &m, const FqW9 &A) {
    FqW9 r; uint64_t c = 0;
    for (int i = 0; i < 8; i++) { const uint64_t s = (uint64_t)m.l[i] + A.l[i] + c; r.l[i] = (uint32_t)s & M29; c = s >> 29; }
    r.l[8] = (uint32_t)((uint64_t)m.l[8] + A.l[8] + c);
    return r;
}
// 128-bit shadows of the column chains: the largest value the 64-bit accumulator would have to hold
static u128 shadow_mulw_add(const FqW9 &a, const FqW9 &b, const FqW9 &A) {
    uint32_t m[9]; u128 acc = 0, top = 0;
    for (int k = 0; k < 17; k++) {
        for (int i = (k < 9 ? 0 : k - 8); i <= (k < 9 ? k : 8); i++) acc += (u128)a.l[k - i] * b.l[i];
        for (int i = (k < 9 ? 0 : k - 8); i <= (k < 9 ? k - 1 : 8); i++) acc += (u128)m[i] * FqW::P29[k - i];
        if (k < 9) { m[k] = ((uint32_t)acc * FqW::INV29) & M29; acc += (u128)m[k] * FqW::P29[0]; } else acc += A.l[k - 9];
        if (acc > top) top = acc;
        acc >>= 29;
    }
    return top;
}
static u128 shadow_mul2addw(const FqW9 &a, const FqW9 &b, const FqW9 &c, const FqW9 &d) {
    uint32_t m[9]; u128 acc = 0, top = 0;
    for (int k = 0; k < 17; k++) {
        for (int i = (k < 9 ? 0 : k - 8); i <= (k < 9 ? k : 8); i++) acc += (u128)a.l[k - i] * b.l[i] + (u128)c.l[k - i] * d.l[i];
        for (int i = (k < 9 ? 0 : k - 8); i <= (k < 9 ? k - 1 : 8); i++) acc += (u128)m[i] * FqW::P29[k - i];
        if (k < 9) { m[k] = ((uint32_t)acc * FqW::INV29) & M29; acc += (u128)m[k] * FqW::P29[0]; }
        if (acc > top) top = acc;
        acc >>= 29;
    }
    return top;
}

// ---- reference copy of the mixed addition as it was (separate products, padded subtractions, normw; is_inf tests)
static void ref_add_mixed(XyzzW &acc, const AffW &q, bool neg_q) {
    if (is_inf(q)) return;
    if (is_inf(acc)) { acc.x = q.x; acc.y = neg_q ? neg2(q.y) : q.y; acc.zz = w_one<FqW>(); acc.zzz = w_one<FqW>(); return; }
    FqW9 u2, s2;
    mulw2<FqW>(q.x, acc.zz, q.y, acc.zzz, u2, s2);
    FqW9 p = sub6(u2, acc.x);
    FqW9 r;
    {
        const uint32_t m = neg_q ? 0xffffffffu : 0u;
        for (int i = 0; i < 9; i++) r.l[i] = FqW::PAD8[i] - acc.y.l[i] + ((s2.l[i] ^ m) - m);
        r = normw(r);
    }
    if (maybe_zero_mod_p(p)) { xyzzw_add_mixed_special(acc, q, neg_q, p, r); return; }
    FqW9 pp, rr, ppp, qq;
    sqrw2<FqW>(p, r, pp, rr);
    mulw2<FqW>(p, pp, acc.x, pp, ppp, qq);
    FqW9 x3;
    {
        for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
        x3 = normw(x3);
    }
    FqW9 zz3, zzz3;
    mulw2<FqW>(acc.zz, pp, acc.zzz, ppp, zz3, zzz3);
    acc.y = mul2addw<FqW>(r, sub6(qq, x3), acc.y, neg2(ppp));
    acc.x = x3; acc.zz = zz3; acc.zzz = zzz3;
}

static G1Affine to_aff(const G1Xyzz &p) {
    G1Affine a; if (is_inf(p)) { a.x = Fq::zero(); a.y = Fq::zero(); return a; }
    Fq i = inv(mul(p.zz, p.zzz)); a.x = mul(p.x, mul(i, p.zzz)); a.y = mul(p.y, mul(i, p.zz)); return a; }
static AffW aff_to_w(const G1Affine &a) { AffW r; r.x = csub_p(w_from_s(unpack<FqW>(a.x))); r.y = csub_p(w_from_s(unpack<FqW>(a.y))); return r; }
static G1Xyzz exportw(const XyzzW &p) {
    if (is_inf(p)) return xyzz_identity();
    G1Xyzz r; r.x = pack<FqParams>(s_from_w(p.x)); r.y = pack<FqParams>(s_from_w(p.y)); r.zz = pack<FqParams>(s_from_w(p.zz)); r.zzz = pack<FqParams>(s_from_w(p.zzz)); return r; }

static int ebad = 0;
static FqW9 SIX_P, P13_10;
// one addition by both forms from the same accumulator; returns the new form's result
static XyzzW both(const XyzzW &acc, const AffW &q, bool neg, const char *what, int it, bool check_bounds = true) {
    XyzzW want = acc, got = acc;
    bool fresh = is_inf(acc);
    ref_add_mixed(want, q, neg);
    xyzzw_add_mixed_flag(got, fresh, q, neg);
    bool ok = fresh == is_inf(got) && is_inf(got) == is_inf(want);
    const FqW9 *g[4] = {&got.x, &got.y, &got.zz, &got.zzz}, *w[4] = {&want.x, &want.y, &want.zz, &want.zzz};
    for (int c = 0; c < 4 && ok; c++) {
        if (!neg) ok = same(*g[c], *w[c]);                                               // the same integers
        else ok = is_inf(got) ? same(*g[c], *w[c]) : same(reduce_full(*g[c]), reduce_full(*w[c]));
        for (int i = 0; i < 8; i++) if (g[c]->l[i] > M29) ok = false;                      // normalised
    }
    if (ok && check_bounds && !is_inf(got)) ok = less(got.x, SIX_P) && less(got.y, SIX_P) && less(got.zz, P13_10) && less(got.zzz, P13_10);
    if (!ok) { ebad++; if (ebad < 8) printf("mixed addition mismatch: %s, case %d, neg %d\n", what, it, (int)neg); }
    return got;
}

int main() {
    int bad = 0;
    SIX_P = p_times(6); P13_10 = p_times(13, 10);
    const u128 LIMIT = (u128)1 << 64;
    // ---------------------------------------------------------------- 1. mulw2_add
    for (int it = 0; it < 30000; it++) {
        FqW9 a0 = rnd_w(), b0 = rnd_w(), a1 = rnd_w(), b1 = rnd_w(), x = rnd_w(), y = rnd_w(), A0, A1;
        const int kind = it & 7;
        x = addn(x, p_times(rnd() % 5));                                                   // accumulator coordinates: < 6p
        y = addn(y, p_times(rnd() % 5));
        if (kind == 1) { x = minus_one(SIX_P); y = minus_one(SIX_P); b0 = minus_one(P13_10); b1 = minus_one(P13_10); }     // at their stated multiples of p
        if (kind == 2) { x = w_zero<FqW>(); y = w_zero<FqW>(); }
        for (int i = 0; i < 9; i++) { A0.l[i] = FqW::PAD6[i] - x.l[i]; A1.l[i] = FqW::PAD8[i] - y.l[i]; }    // as the mixed addition forms them
        if (kind == 3) for (int i = 0; i < 9; i++) a1.l[i] = FqW::PAD2[i] - a1.l[i];       // 2p - y as left operand, not normalised
        if (kind == 4) { for (int i = 0; i < 8; i++) { a0.l[i] = MULW_A_LIMB_MAX; a1.l[i] = MULW_A_LIMB_MAX; b0.l[i] = M29; b1.l[i] = M29; } a0.l[8] = a1.l[8] = b0.l[8] = b1.l[8] = 0x00ffffffu; }
        if (kind == 5) { for (int i = 0; i < 8; i++) { A0.l[i] = 0xffffffffu; A1.l[i] = 0xffffffffu; } }     // addend limbs at 2^32 - 1
        if (kind == 6) { for (int i = 0; i < 8; i++) { a0.l[i] = MULW_A_LIMB_MAX; a1.l[i] = MULW_A_LIMB_MAX; b0.l[i] = M29; b1.l[i] = M29; A0.l[i] = 0xffffffffu; A1.l[i] = 0xffffffffu; }
                         a0.l[8] = a1.l[8] = b0.l[8] = b1.l[8] = 0x00ffffffu; }           // everything at its bound at once
        FqW9 r0, r1;
        mulw2_add<FqW>(a0, b0, A0, a1, b1, A1, r0, r1);
        const FqW9 w0 = add_norm64(mulw(a0, b0), A0), w1 = add_norm64(mulw(a1, b1), A1);
        if (!same(r0, w0) || !same(r1, w1)) { bad++; if (bad < 8) printf("mulw2_add mismatch at %d (kind %d)\n", it, kind); }
        if (kind < 5) {                                                                    // the replaced code itself, where its limbs fit 32 bits
            const FqW9 o0 = normw(addw(mulw(a0, b0), A0)), o1 = normw(addw(mulw(a1, b1), A1));
            if (!same(r0, o0) || !same(r1, o1)) { bad++; if (bad < 8) printf("mulw2_add differs from normw(addw(mulw)) at %d (kind %d)\n", it, kind); }
        }
        if (kind <= 1) {                                                                   // ... and the subtraction helpers the call sites used
            if (!same(r0, sub6(mulw(a0, b0), x))) { bad++; if (bad < 8) printf("mulw2_add differs from sub6(mulw) at %d\n", it); }
        }
        if (shadow_mulw_add(a0, b0, A0) >= LIMIT || shadow_mulw_add(a1, b1, A1) >= LIMIT) { bad++; if (bad < 8) printf("mulw2_add: a column exceeds 64 bits at %d (kind %d)\n", it, kind); }
    }
    // ---------------------------------------------------------------- 2. mul2addw with the raw Q - X3 + 6p and 2p - PPP (2^29-bias pads)
    {
        FqW9 n2, n6;
        for (int i = 0; i < 9; i++) { n2.l[i] = FqW::PAD2N[i]; n6.l[i] = FqW::PAD6N[i]; }
        if (!same(normw(n2), p_times(2)) || !same(normw(n6), p_times(6))) { bad++; printf("PAD2N / PAD6N are not 2p / 6p\n"); }
    }
    for (int it = 0; it < 30000; it++) {
        FqW9 r = rnd_w(), qq = rnd_w(), x3 = rnd_w(), y = rnd_w(), ppp = rnd_w(), t, d;
        r = addn(r, p_times(rnd() % 9)); x3 = addn(x3, p_times(rnd() % 5)); y = addn(y, p_times(rnd() % 5));
        const int kind = it & 3;
        if (kind == 1) { ppp = w_zero<FqW>(); x3 = w_zero<FqW>(); }                        // the largest limbs of both differences: the pads' own, plus Q's
        if (kind == 2) { ppp = w_zero<FqW>(); x3 = w_zero<FqW>(); for (int i = 0; i < 8; i++) { r.l[i] = M29; qq.l[i] = M29; y.l[i] = M29; } r.l[8] = y.l[8] = 0x00ffffffu; }    // every limb at its bound
        if (kind == 3) { for (int i = 0; i < 8; i++) { x3.l[i] = M29; ppp.l[i] = M29; } x3.l[8] = minus_one(p_times(11, 2)).l[8] - 1; ppp.l[8] = p_times(1).l[8]; }   // the subtrahends' largest limbs: no limb of a difference goes negative
        for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; d.l[i] = FqW::PAD2N[i] - ppp.l[i]; }
        for (int i = 0; i < 9; i++) if (t.l[i] > 1450000000u || d.l[i] > 1020000000u) { bad++; if (bad < 8) printf("a raw difference exceeds its documented limb bound at %d (kind %d)\n", it, kind); break; }
        const FqW9 got = mul2addw<FqW>(r, t, y, d), want = mul2addw<FqW>(r, sub6(qq, x3), y, neg2(ppp));
        if (!same(got, want)) { bad++; if (bad < 8) printf("mul2addw with the raw differences differs at %d (kind %d)\n", it, kind); }
        const u128 top = shadow_mul2addw(r, t, y, d);
        if (top >= LIMIT - (LIMIT >> 3)) { bad++; if (bad < 8) printf("mul2addw: a column within 1/8 of 2^64 at %d (kind %d)\n", it, kind); }
    }
    printf("addend forms: %d mismatches\n", bad);
    // ---------------------------------------------------------------- 3. the mixed addition
    // (a) arbitrary field elements as coordinates (the formulas are polynomial identities), accumulator coordinates up to their bounds
    int cases = 0;
    for (int it = 0; it < 60000; it++, cases++) {
        XyzzW acc; AffW q;
        acc.x = addn(rnd_w(), p_times(rnd() % 5)); acc.y = addn(rnd_w(), p_times(rnd() % 5));
        acc.zz = rnd_w(); acc.zzz = rnd_w();
        q.x = csub_p(rnd_w()); q.y = csub_p(rnd_w());
        if ((it & 15) == 1) { acc.x = minus_one(SIX_P); acc.y = minus_one(SIX_P); acc.zz = minus_one(P13_10); acc.zzz = minus_one(P13_10); }
        if ((it & 15) == 2) { acc.x = w_zero<FqW>(); acc.y = w_zero<FqW>(); }                  // (zz != 0: not the identity)
        if ((it & 15) == 3) acc = xyzzw_identity();
        if ((it & 15) == 4) { q.x = minus_one(p_times(1)); q.y = minus_one(p_times(1)); }
        both(acc, q, (it >> 4) & 1, "random coordinates", it);
    }
    // (b) a walk over curve points with the edge cases: P + P, P - P, the accumulator at the identity, y negated
    G1Affine g; g.x = from_u64<FqParams>(1); g.y = from_u64<FqParams>(2);
    AffW ptsw[16];
    { G1Xyzz t = xyzz_from_affine(g); for (int i = 0; i < 16; i++) { ptsw[i] = aff_to_w(to_aff(t)); t = xyzz_double(t); xyzz_add_mixed(t, g, false); } }
    XyzzW acc = xyzzw_identity();
    for (int it = 0; it < 45000; it++, cases++) {
        const int k = rnd() & 15, op = rnd() % 23; const bool ng = rnd() & 1;
        if (op < 20) acc = both(acc, ptsw[k], ng, "walk", it);
        else if (op == 20 || op == 21) {                                                   // acc +- acc: doubling / identity through the special path
            if (is_inf(acc)) { acc = both(acc, ptsw[k], ng, "walk from the identity", it); continue; }
            const AffW cw = aff_to_w(to_aff(exportw(acc)));
            acc = both(acc, cw, op == 21, op == 21 ? "P - P" : "P + P", it);
            if (op == 21) { if (!is_inf(acc)) { ebad++; printf("P - P is not the identity at %d\n", it); } }
        } else if (op == 22) {                                                             // the same with the sign on the affine operand
            if (is_inf(acc)) continue;
            AffW cw = aff_to_w(to_aff(exportw(acc)));
            cw.y = csub_p(neg2(cw.y));
            acc = both(acc, cw, ng, ng ? "P + P (negated operand)" : "P - P (negated operand)", it);
        }
    }
    // the walk has stayed on XYZZ coordinates: zz^3 == zzz^2
    if (!is_inf(acc)) { const FqW9 a = reduce_full(mulw(sqrw(acc.zz), acc.zz)), b = reduce_full(sqrw(acc.zzz)); if (!same(a, b)) { ebad++; printf("zz^3 != zzz^2 at the end of the walk\n"); } }
    printf("mixed addition: %d mismatches in %d cases\n", ebad, cases);
    return (bad + ebad) ? 1 : 0;
}
