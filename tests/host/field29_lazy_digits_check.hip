// Host-side check of the products with lazy Montgomery digits (field29_dev.h: mulw2_lz, sqrw2_lz, mulw2_add_lz, mul2addw_lz — the digits
// m_0..m_7 of the reduction left unmasked) and of the two additions built on them (ec29_dev.h: xyzzw_add_mixed_flag, xyzzw_add_pairs).
// Built and run by tests/test_field29_lazy_digits_host.py with hipcc; needs no GPU.  A stand-alone program: it may also be built with
// -Xarch_host -fsanitize=address,undefined and run directly.
//   1. Every form, in the instantiations the two additions use, against its masked form on the same operands: operands with every limb at
//      its DECLARED bound (the bounds the static_assert of the form is evaluated at), > 10^5 random operands in the shapes the additions feed
//      in, and operands built so that the multiplier m~ passes 2^261 (the masked m below 2^232 + ...: its top digit wraps once an unmasked
//      digit below it carries).  Each chain is shadowed in 128 bits with the same unmasked digits.  Asserted: no column reaches 2^64 (the
//      largest one seen is printed beside the compile-time worst case, which it may not exceed); the form returns the shadow's limbs; output
//      limbs 0..7 are below 2^29; result - masked result is 0 or p exactly (both must occur); m~ < 2^261 + 2^235, which is what puts the
//      result below the masked form's bound a*b / 2^261 + p by less than 2^-26 p.
//   2. Both additions, new against old (xyzzw_add_mixed_flag as it was with the masked forms, kept below - both the form with the
//      accumulator's own x, y and xyzzw_add_mixed_nflag, which carries them negated: from the flipped accumulator, and carried by itself along
//      the walk, flipped back for the comparison; xyzzw_add for the full addition),
//      > 10^5 cases each: random coordinates up to the accumulator's bounds, walks over curve points with P = +-Q, a fresh accumulator, an
//      identity operand, y negated.  Equal after full reduction in every coordinate, equal identity flags, normalised limbs, coordinates
//      below their documented bounds.
#include "ec29_dev.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
using namespace plk;
typedef unsigned __int128 u128;
static uint64_t rs = 0x9e3779b97f4a7c15ULL;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 16); }
static Fq rnd_fq() { Fq a; for (int i = 0; i < 8; i++) a.l[i] = rnd(); a.l[7] &= 0x0fffffff; return a; }   // < 2^252 < p
static FqW9 rnd_w() { return w_from_s(unpack<FqW>(rnd_fq())); }                                          // < 1.1p, normalised
static bool same(const FqW9 &a, const FqW9 &b) { for (int i = 0; i < 9; i++) if (a.l[i] != b.l[i]) return false; return true; }
static bool less(const FqW9 &a, const FqW9 &b) { for (int i = 8; i >= 0; i--) if (a.l[i] != b.l[i]) return a.l[i] < b.l[i]; return false; }
static FqW9 p_times(uint32_t num, uint32_t den = 1) {
    uint64_t t[9], c = 0;
    for (int i = 0; i < 9; i++) { c += (uint64_t)num * FqW::P29[i]; t[i] = c & M29; c >>= 29; }
    t[8] += c << 29;
    FqW9 r; uint64_t rem = 0;
    for (int i = 8; i >= 0; i--) { const uint64_t v = (rem << 29) + t[i]; r.l[i] = (uint32_t)(v / den); rem = v % den; }
    return r;
}
static FqW9 minus_one(FqW9 a) { int i = 0; while (a.l[i] == 0) { a.l[i] = M29; i++; } a.l[i]--; return a; }
static FqW9 at(const Limbs9 &b) { FqW9 r; for (int i = 0; i < 9; i++) r.l[i] = b.l[i]; return r; }
static FqW9 unit() { FqW9 r = w_zero<FqW>(); r.l[0] = 1; return r; }
// new - old as integers (both normalised in limbs 0..7): 0 -> 0, p -> 1, anything else -> -1
static int diff_class(const FqW9 &nw, const FqW9 &old) {
    int64_t c = 0; bool zero = true, isp = true;
    for (int i = 0; i < 9; i++) {
        const int64_t s = (int64_t)nw.l[i] - (int64_t)old.l[i] + c;
        const int64_t limb = i < 8 ? (s & (int64_t)M29) : s;
        c = i < 8 ? (s >> 29) : 0;
        if (limb != 0) zero = false;
        if (limb != (int64_t)FqW::P29[i]) isp = false;
    }
    return zero ? 0 : isp ? 1 : -1;
}

// ---- the 128-bit shadow of a column chain a*b + c*d + m~*p (+ addend), digits of lz unmasked; sq: a squaring of a (b, c, d unused)
struct Shadow { u128 top; FqW9 r; bool m_ok; uint32_t m[9]; };
static Shadow shadow(const FqW9 &a, const FqW9 &b, const FqW9 *c, const FqW9 *d, const FqW9 *A, unsigned lz, bool sq) {
    Shadow s; s.top = 0;
    u128 acc = 0;
    for (int k = 0; k < 17; k++) {
        const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8;
        if (sq) {
            for (int i = lo; 2 * i < k; i++) acc += (u128)(uint32_t)(a.l[k - i] << 1) * a.l[i];
            if (k % 2 == 0) acc += (u128)a.l[k / 2] * a.l[k / 2];
        } else for (int i = lo; i <= hi; i++) { acc += (u128)a.l[k - i] * b.l[i]; if (c) acc += (u128)c->l[k - i] * d->l[i]; }
        for (int i = lo; i <= (k < 9 ? k - 1 : 8); i++) acc += (u128)s.m[i] * FqW::P29[k - i];
        if (k < 9) { s.m[k] = (uint32_t)acc * FqW::INV29; if (!lazy_digit(lz, k)) s.m[k] &= M29; acc += (u128)s.m[k] * FqW::P29[0]; }
        else if (A) acc += A->l[k - 9];
        if (acc > s.top) s.top = acc;
        if (k >= 9) s.r.l[k - 9] = (uint32_t)acc & M29;
        acc >>= 29;
    }
    s.r.l[8] = (uint32_t)acc + (A ? A->l[8] : 0);
    // m~ = sum m_k 2^(29 k) < 2^261 + 2^235: carry the digits into ten limbs; limb 9 is 0, or 1 with limb 8 below 2^3 (2^235 = 2^3 * 2^232)
    uint64_t cy = 0, l8 = 0;
    for (int k = 0; k < 9; k++) { cy += s.m[k]; if (k == 8) l8 = cy & M29; cy >>= 29; }
    s.m_ok = cy == 0 || (cy == 1 && l8 < 8);
    return s;
}

static int bad = 0, cases1 = 0, plus_p[4] = {0, 0, 0, 0}, same_int[4] = {0, 0, 0, 0};
static u128 top_seen[4] = {0, 0, 0, 0};
static const char *FORM[4] = {"mulw2_lz", "sqrw2_lz", "mulw2_add_lz", "mul2addw_lz"};
static void fail(const char *what, int form, const char *kind) { bad++; if (bad < 12) printf("%s: %s (%s, case %d)\n", FORM[form], what, kind, cases1); }
// one chain's result `got` against its shadow and against the masked form's `old`
static void judge(int form, const Shadow &s, const FqW9 &got, const FqW9 &old, const char *kind) {
    if (s.top > top_seen[form]) top_seen[form] = s.top;
    if (s.top >> 64) fail("a column exceeds 64 bits", form, kind);
    if (!same(got, s.r)) fail("the form's limbs are not the shadow's", form, kind);
    for (int i = 0; i < 8; i++) if (got.l[i] > M29) { fail("an output limb is not normalised", form, kind); break; }
    if (!s.m_ok) fail("the multiplier exceeds 2^261 + 2^235", form, kind);
    const int d = diff_class(got, old);
    if (d < 0) fail("result - masked result is neither 0 nor p", form, kind);
    else if (d) plus_p[form]++; else same_int[form]++;
}
// the instantiations of the two additions
#define MUL2(a0, b0, a1, b1, r0, r1) mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm>(a0, b0, a1, b1, r0, r1)
#define SQR2(x0, x1, r0, r1) sqrw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm>(x0, x1, r0, r1)
#define MUL2ADD(a0, b0, A0, a1, b1, A1, r0, r1) mulw2_add_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbAny, LbSignedY, LbNorm, LbAny>(a0, b0, A0, a1, b1, A1, r0, r1)
static void check_mul2(const FqW9 &a0, const FqW9 &b0, const FqW9 &a1, const FqW9 &b1, const char *kind) {
    FqW9 r0, r1, o0, o1;
    MUL2(a0, b0, a1, b1, r0, r1);
    mulw2<FqW>(a0, b0, a1, b1, o0, o1);
    judge(0, shadow(a0, b0, nullptr, nullptr, nullptr, LZ_ALL, false), r0, o0, kind);
    judge(0, shadow(a1, b1, nullptr, nullptr, nullptr, LZ_ALL, false), r1, o1, kind);
    cases1++;
}
static void check_sqr2(const FqW9 &x0, const FqW9 &x1, const char *kind) {
    FqW9 r0, r1, o0, o1;
    SQR2(x0, x1, r0, r1);
    sqrw2<FqW>(x0, x1, o0, o1);
    judge(1, shadow(x0, x0, nullptr, nullptr, nullptr, LZ_ALL, true), r0, o0, kind);
    judge(1, shadow(x1, x1, nullptr, nullptr, nullptr, LZ_ALL, true), r1, o1, kind);
    cases1++;
}
static void check_mul2add(const FqW9 &a0, const FqW9 &b0, const FqW9 &A0, const FqW9 &a1, const FqW9 &b1, const FqW9 &A1, const char *kind) {
    FqW9 r0, r1, o0, o1;
    MUL2ADD(a0, b0, A0, a1, b1, A1, r0, r1);
    mulw2_add<FqW>(a0, b0, A0, a1, b1, A1, o0, o1);
    judge(2, shadow(a0, b0, nullptr, nullptr, &A0, LZ_ALL, false), r0, o0, kind);
    judge(2, shadow(a1, b1, nullptr, nullptr, &A1, LZ_ALL, false), r1, o1, kind);
    cases1++;
}
static void check_mul2addw(const FqW9 &a, const FqW9 &b, const FqW9 &c, const FqW9 &d, const char *kind) {
    const FqW9 r = WMA_LZ(a, b, c, d), o = mul2addw<FqW>(a, b, c, d);
    judge(3, shadow(a, b, &c, &d, nullptr, LZ_ALL, false), r, o, kind);
    cases1++;
}

// ---- operands whose masked multiplier m has its top digit below 8, so that m~ passes 2^261 when the unmasked digit 7 carries into it
// a = -m * p mod 2^261 for a random m < 2^232: the product a * 1 has exactly this m
static FqW9 wrap_operand() {
    uint32_t m[9]; for (int i = 0; i < 8; i++) m[i] = rnd() & M29; m[8] = 0;
    uint32_t lo[9];
    u128 acc = 0;
    for (int k = 0; k < 9; k++) { for (int i = 0; i <= k; i++) acc += (u128)m[i] * FqW::P29[k - i]; lo[k] = (uint32_t)acc & M29; acc >>= 29; }
    FqW9 a; int64_t c = 0;                                      // 2^261 - lo
    for (int k = 0; k < 9; k++) { const int64_t s = c - (int64_t)lo[k]; a.l[k] = (uint32_t)(s & (int64_t)M29); c = s >> 29; }
    return a;
}
// the same for a squaring: x = v + u 2^116 + w 2^232 has x^2 = v^2 + 2uv 2^116 + (u^2 + 2vw) 2^232 (mod 2^261), so w moves the top digit of m
// by -2 v w p^-1 (mod 2^29): solved for a top digit of 0 or 1 (v odd)
static uint32_t inv_odd(uint32_t a) { uint32_t x = a; for (int i = 0; i < 5; i++) x *= 2 - a * x; return x; }
static FqW9 wrap_square_operand() {
    FqW9 x = w_zero<FqW>();
    x.l[0] = (rnd() & M29) | 1; x.l[4] = rnd() & M29;
    const uint32_t t = shadow(x, x, nullptr, nullptr, nullptr, 0, true).m[8];
    const uint32_t g = x.l[0] * FqW::PINV0;                     // m_8 = t - 2 g w (mod 2^29)
    x.l[8] = ((t >> 1) * inv_odd(g)) & ((1u << 28) - 1);
    return x;
}

// ---- the mixed addition as it was, on the masked forms
static void old_add_mixed_flag(XyzzW &acc, bool &fresh, const AffW &q, bool neg_q) {
    if (fresh) { acc.x = q.x; acc.y = neg_q ? neg2(q.y) : q.y; acc.zz = w_one<FqW>(); acc.zzz = w_one<FqW>(); fresh = false; return; }
    FqW9 p, r, yq, ax, ay;
    for (int i = 0; i < 9; i++) { ax.l[i] = FqW::PAD6[i] - acc.x.l[i]; ay.l[i] = FqW::PAD8[i] - acc.y.l[i]; yq.l[i] = neg_q ? FqW::PAD2[i] - q.y.l[i] : q.y.l[i]; }
    mulw2_add<FqW>(q.x, acc.zz, ax, yq, acc.zzz, ay, p, r);
    if (maybe_zero_mod_p(p)) { AffW t; t.x = q.x; t.y = normw(yq); xyzzw_add_mixed_special(acc, t, false, p, r); fresh = is_inf(acc); return; }
    FqW9 pp, rr, ppp, qq, x3, zz3, zzz3, t, nppp;
    sqrw2<FqW>(p, r, pp, rr);
    mulw2<FqW>(p, pp, acc.x, pp, ppp, qq);
    for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
    x3 = normw(x3);
    mulw2<FqW>(acc.zz, pp, acc.zzz, ppp, zz3, zzz3);
    for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; nppp.l[i] = FqW::PAD2N[i] - ppp.l[i]; }
    acc.y = mul2addw<FqW>(r, t, acc.y, nppp);
    acc.x = x3; acc.zz = zz3; acc.zzz = zzz3;
}

static G1Affine to_aff(const G1Xyzz &p) {
    G1Affine a; if (is_inf(p)) { a.x = Fq::zero(); a.y = Fq::zero(); return a; }
    Fq i = inv(mul(p.zz, p.zzz)); a.x = mul(p.x, mul(i, p.zzz)); a.y = mul(p.y, mul(i, p.zz)); return a; }
static AffW aff_to_w(const G1Affine &a) { AffW r; r.x = csub_p(w_from_s(unpack<FqW>(a.x))); r.y = csub_p(w_from_s(unpack<FqW>(a.y))); return r; }
static G1Xyzz exportw(const XyzzW &p) {
    if (is_inf(p)) return xyzz_identity();
    G1Xyzz r; r.x = pack<FqParams>(s_from_w(p.x)); r.y = pack<FqParams>(s_from_w(p.y)); r.zz = pack<FqParams>(s_from_w(p.zz)); r.zzz = pack<FqParams>(s_from_w(p.zzz)); return r; }

static int mbad = 0, mcases = 0, mspecial = 0, mfresh = 0, fbad = 0, fcases = 0, fhot = 0, fident = 0, not_same_integers = 0;
static FqW9 SIX_P, P13_10;
// new == old after full reduction, identity for identity, normalised limbs, coordinates below the accumulator's bounds
static bool agree(const XyzzW &got, const XyzzW &want, bool check_bounds, bool count_ints = true) {
    if (is_inf(got) != is_inf(want)) return false;
    if (is_inf(got)) return true;
    const FqW9 *g[4] = {&got.x, &got.y, &got.zz, &got.zzz}, *w[4] = {&want.x, &want.y, &want.zz, &want.zzz};
    bool ok = true, ints = true;
    for (int c = 0; c < 4; c++) {
        if (!same(reduce_full(*g[c]), reduce_full(*w[c]))) ok = false;
        if (!same(*g[c], *w[c])) ints = false;
        for (int i = 0; i < 8; i++) if (g[c]->l[i] > M29) ok = false;
    }
    if (!ints && count_ints) not_same_integers++;
    if (check_bounds) ok = ok && less(got.x, SIX_P) && less(got.y, SIX_P) && less(got.zz, P13_10) && less(got.zzz, P13_10);
    return ok;
}
// ncarry: the accumulator of the negated-coordinate form (xyzzw_add_mixed_nflag) as that form itself left it; without one it starts from the flipped acc
static XyzzW both_mixed(const XyzzW &acc, const AffW &q, bool neg, const char *what, XyzzW *ncarry = nullptr) {
    XyzzW want = acc, got = acc;
    bool f0 = is_inf(acc), f1 = f0, f2 = f0;
    mfresh += f0;
    old_add_mixed_flag(want, f0, q, neg);
    xyzzw_add_mixed_flag(got, f1, q, neg);
    XyzzW ngot = ncarry ? *ncarry : (is_inf(acc) ? acc : xyzzw_flip_xy(acc));
    xyzzw_add_mixed_nflag(ngot, f2, q, neg);
    if (ncarry) *ncarry = ngot;
    mcases++;
    bool ok = f0 == f1 && f1 == is_inf(got) && agree(got, want, true);
    ok = ok && f2 == f0 && f2 == is_inf(ngot) && (f2 || (less(ngot.x, SIX_P) && less(ngot.y, SIX_P) && agree(xyzzw_flip_xy(ngot), want, true, false)));
    if (!ok) { mbad++; if (mbad < 8) printf("mixed addition mismatch: %s (case %d, neg %d)\n", what, mcases, (int)neg); }
    return got;
}
static XyzzW both_full(const XyzzW &a, const XyzzW &b, const char *what, bool check_bounds = true) {
    XyzzW want = a, got = a;
    xyzzw_add(want, b);
    xyzzw_add_pairs(got, b);
    fcases++;
    if (is_inf(got)) fident++; else if (!is_inf(a) && !is_inf(b)) fhot++;
    if (!agree(got, want, check_bounds)) { fbad++; if (fbad < 8) printf("full addition mismatch: %s (case %d)\n", what, fcases); }
    return got;
}

int main() {
    SIX_P = p_times(6); P13_10 = p_times(13, 10);
    const double TWO64 = 18446744073709551616.0;
    // ---------------------------------------------------------------- 1. the forms
    // the compile-time worst case of every instantiation (what its static_assert evaluates), to set beside the columns seen
    const ColBound cb[4] = {lazy_col_bound(LbNorm::B, LbNorm::B, LbNone::B, LbNone::B, LbNone::B, FqW::P29, LZ_ALL),
                            lazy_col_bound(LbNorm::B, LbNorm::B, LbNone::B, LbNone::B, LbNone::B, FqW::P29, LZ_ALL),
                            lazy_col_bound(LbSignedY::B, LbNorm::B, LbNone::B, LbNone::B, LbAny::B, FqW::P29, LZ_ALL),
                            lazy_col_bound(LbNorm::B, LbT::B, LbNorm::B, LbNppp::B, LbNone::B, FqW::P29, LZ_ALL)};
    // (a) every limb at its declared bound
    {
        const FqW9 n = at(LbNorm::B), any = at(LbAny::B), sy = at(LbSignedY::B), t = at(LbT::B), np = at(LbNppp::B);
        check_mul2(n, n, n, n, "limbs at the declared bounds");
        check_sqr2(n, n, "limbs at the declared bounds");
        check_mul2add(n, n, any, sy, n, any, "limbs at the declared bounds");
        check_mul2addw(n, t, n, np, "limbs at the declared bounds");
        // ... and with the lower limbs at the bound under a top limb as small as the values really are (results stay far below 2^261)
        FqW9 n6 = n, n13 = n, sy2 = sy, t2 = t, np2 = np;
        n6.l[8] = SIX_P.l[8]; n13.l[8] = P13_10.l[8]; sy2.l[8] = FqW::PAD2[8]; t2.l[8] = FqW::PAD6N[8] + P13_10.l[8]; np2.l[8] = FqW::PAD2N[8];
        check_mul2(n6, n13, n6, n13, "lower limbs at the declared bounds");
        check_sqr2(n6, n6, "lower limbs at the declared bounds");
        FqW9 a6, a8; for (int i = 0; i < 9; i++) { a6.l[i] = FqW::PAD6[i]; a8.l[i] = FqW::PAD8[i]; }
        check_mul2add(n13, n13, a6, sy2, n13, a8, "lower limbs at the declared bounds");
        check_mul2addw(n6, t2, n6, np2, "lower limbs at the declared bounds");
    }
    // (b) random operands in the shapes the additions feed in
    for (int it = 0; it < 30000; it++) {
        FqW9 x = addn(rnd_w(), p_times(rnd() % 5)), y = addn(rnd_w(), p_times(rnd() % 5)), zz = rnd_w(), zzz = rnd_w();
        FqW9 qx = csub_p(rnd_w()), qy = csub_p(rnd_w()), ax, ay, yq;
        const bool neg = it & 1;
        if ((it & 15) == 2) { x = minus_one(SIX_P); y = minus_one(SIX_P); zz = minus_one(P13_10); zzz = minus_one(P13_10); }
        if ((it & 15) == 4) { for (int i = 0; i < 8; i++) { x.l[i] = y.l[i] = zz.l[i] = zzz.l[i] = M29; } x.l[8] = y.l[8] = SIX_P.l[8] - 1; zz.l[8] = zzz.l[8] = P13_10.l[8] - 1; }
        if ((it & 15) == 6) { qy = w_zero<FqW>(); }              // 2p - y at the pad's own limbs
        for (int i = 0; i < 9; i++) { ax.l[i] = FqW::PAD6[i] - x.l[i]; ay.l[i] = FqW::PAD8[i] - y.l[i]; yq.l[i] = neg ? FqW::PAD2[i] - qy.l[i] : qy.l[i]; }
        check_mul2add(qx, zz, ax, yq, zzz, ay, "P, R of the mixed addition");
        FqW9 p, r, pp, rr, ppp, qq, x3, t, nppp;
        MUL2ADD(qx, zz, ax, yq, zzz, ay, p, r);
        check_sqr2(p, r, "PP, RR");
        SQR2(p, r, pp, rr);
        check_mul2(p, pp, x, pp, "PPP, Q");
        MUL2(p, pp, x, pp, ppp, qq);
        check_mul2(zz, pp, zzz, ppp, "ZZ3, ZZZ3");
        check_mul2(x, zz, y, zzz, "U1, S1 of the full addition");
        for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
        x3 = normw(x3);
        for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; nppp.l[i] = FqW::PAD2N[i] - ppp.l[i]; }
        for (int i = 0; i < 9; i++) if (t.l[i] > LbT::B.l[i] || nppp.l[i] > LbNppp::B.l[i] || yq.l[i] > LbSignedY::B.l[i]) { bad++; printf("an operand exceeds its declared limb bound\n"); break; }
        check_mul2addw(r, t, y, nppp, "the fused Y3");
    }
    // (c) multipliers that pass 2^261: the result is the masked form's plus p
    for (int it = 0; it < 400; it++) {
        const FqW9 a0 = wrap_operand(), a1 = wrap_operand(), one = unit(), z = w_zero<FqW>();
        check_mul2(a0, one, a1, one, "top digit of m below 8");
        FqW9 A0 = rnd_w(), A1 = rnd_w();
        check_mul2add(a0, one, A0, a1, one, A1, "top digit of m below 8");
        check_mul2addw(a0, one, z, z, "top digit of m below 8");
        check_sqr2(wrap_square_operand(), wrap_square_operand(), "top digit of m below 8");
    }
    for (int f = 0; f < 4; f++) {
        printf("%s: %d results equal to the masked form's, %d larger by p; largest column %.4f * 2^64 (compile-time worst case %.4f * 2^64, fits: %d)\n",
               FORM[f], same_int[f], plus_p[f], (double)top_seen[f] / TWO64, (double)cb[f].worst / TWO64, (int)cb[f].fits);
        if (plus_p[f] == 0 || same_int[f] == 0) { bad++; printf("%s: one of the two outcomes was never seen\n", FORM[f]); }
        if (!cb[f].fits || top_seen[f] > (u128)cb[f].worst) { bad++; printf("%s: a column seen exceeds the compile-time worst case\n", FORM[f]); }
    }
    printf("lazy forms: %d failures in %d calls\n", bad, cases1);
    // ---------------------------------------------------------------- 2. the additions
    // (a) arbitrary field elements as coordinates (the formulas are polynomial identities), up to the accumulator's bounds
    for (int it = 0; it < 60000; it++) {
        XyzzW acc; AffW q;
        acc.x = addn(rnd_w(), p_times(rnd() % 5)); acc.y = addn(rnd_w(), p_times(rnd() % 5)); acc.zz = rnd_w(); acc.zzz = rnd_w();
        q.x = csub_p(rnd_w()); q.y = csub_p(rnd_w());
        if ((it & 15) == 1) { acc.x = minus_one(SIX_P); acc.y = minus_one(SIX_P); acc.zz = minus_one(P13_10); acc.zzz = minus_one(P13_10); }
        if ((it & 15) == 2) { acc.x = w_zero<FqW>(); acc.y = w_zero<FqW>(); }                  // (zz != 0: not the identity)
        if ((it & 15) == 3) acc = xyzzw_identity();                                            // a fresh accumulator
        if ((it & 15) == 4) { q.x = minus_one(p_times(1)); q.y = minus_one(p_times(1)); }
        if ((it & 15) == 5) { for (int i = 0; i < 8; i++) { acc.x.l[i] = acc.y.l[i] = acc.zz.l[i] = acc.zzz.l[i] = M29; } acc.x.l[8] = acc.y.l[8] = SIX_P.l[8] - 1; acc.zz.l[8] = acc.zzz.l[8] = P13_10.l[8] - 1; }
        both_mixed(acc, q, (it >> 4) & 1, "random coordinates");
    }
    for (int it = 0; it < 40000; it++) {
        XyzzW a, b;
        a.x = addn(rnd_w(), p_times(rnd() % 5)); a.y = addn(rnd_w(), p_times(rnd() % 5)); a.zz = rnd_w(); a.zzz = rnd_w();
        b.x = addn(rnd_w(), p_times(rnd() % 5)); b.y = addn(rnd_w(), p_times(rnd() % 5)); b.zz = rnd_w(); b.zzz = rnd_w();
        const int kind = it & 15;
        if (kind == 1) { a.x = minus_one(SIX_P); a.y = minus_one(SIX_P); a.zz = minus_one(P13_10); a.zzz = minus_one(P13_10); }
        if (kind == 2) { b.x = minus_one(SIX_P); b.y = minus_one(SIX_P); b.zz = minus_one(P13_10); b.zzz = minus_one(P13_10); }
        if (kind == 3) { for (int i = 0; i < 8; i++) { a.x.l[i] = a.y.l[i] = a.zz.l[i] = a.zzz.l[i] = b.x.l[i] = b.zz.l[i] = M29; } a.x.l[8] = a.y.l[8] = b.x.l[8] = SIX_P.l[8] - 1; a.zz.l[8] = a.zzz.l[8] = b.zz.l[8] = P13_10.l[8] - 1; }
        if (kind == 8) a = xyzzw_identity();
        if (kind == 9) b = xyzzw_identity();
        both_full(a, b, "random coordinates");
    }
    // (b) walks over curve points: P + P, P - P, the accumulator at the identity, y negated; bucket sums into the full addition
    G1Affine g; g.x = from_u64<FqParams>(1); g.y = from_u64<FqParams>(2);
    AffW ptsw[32];
    { G1Xyzz t = xyzz_from_affine(g); for (int i = 0; i < 32; i++) { ptsw[i] = aff_to_w(to_aff(t)); t = xyzz_double(t); xyzz_add_mixed(t, g, false); } }
    XyzzW acc = xyzzw_identity(), nacc = xyzzw_identity();     // nacc: the same walk in the negated-coordinate form, carried by that form alone
    for (int it = 0; it < 45000; it++) {
        const int k = rnd() & 31, op = rnd() % 23; const bool ng = rnd() & 1;
        if (op < 20 || is_inf(acc)) acc = both_mixed(acc, ptsw[k], ng, "walk", &nacc);
        else {
            AffW cw = aff_to_w(to_aff(exportw(acc)));                                          // acc +- acc through the special path
            if (op == 22) cw.y = csub_p(neg2(cw.y));
            const bool minus = (op == 21) || (op == 22 && !ng);
            acc = both_mixed(acc, cw, op == 22 ? ng : op == 21, minus ? "P - P" : "P + P", &nacc);
            mspecial++;
            if (minus && !is_inf(acc)) { mbad++; printf("P - P is not the identity\n"); }
        }
    }
    auto bucket = [&](int terms) { XyzzW b = xyzzw_identity(); bool fresh = true; for (int j = 0; j < terms; j++) xyzzw_add_mixed_flag(b, fresh, ptsw[rnd() & 31], rnd() & 1); return b; };
    XyzzW pool[16];
    for (int i = 0; i < 16; i++) pool[i] = bucket(1 + (int)(rnd() % 6));
    int fdbl = 0;
    for (int it = 0; it < 70000; it++) {
        const int i = rnd() & 15, j = rnd() & 15, op = rnd() % 16;
        if (op < 7) pool[i] = both_full(pool[i], bucket((int)(rnd() % 5)), "sum + bucket");
        else if (op < 11) pool[i] = both_full(pool[i], pool[j], i == j ? "sum + itself" : "sum + sum");
        else if (op == 11) { XyzzW n = pool[j]; n.y = sub6(w_zero<FqW>(), n.y); const XyzzW z = both_full(pool[j], n, "P - P"); if (!is_inf(z) && !is_inf(pool[j])) { fbad++; printf("P - P is not the identity\n"); } }
        else if (op == 12) {                                                                   // the same point in other coordinates
            if (is_inf(pool[j])) continue;
            const AffW q = aff_to_w(to_aff(exportw(pool[j])));
            XyzzW o; o.x = q.x; o.y = q.y; o.zz = w_one<FqW>(); o.zzz = w_one<FqW>();
            const XyzzW pj = pool[j];
            pool[i] = both_full(pj, o, "P + P (other coordinates)"); fdbl++;
            o.y = neg2(o.y);
            if (!is_inf(both_full(pj, o, "P - P (other coordinates)"))) { fbad++; printf("P - P (other coordinates) is not the identity\n"); }
        }
        else if (op == 13) pool[i] = bucket(1 + (int)(rnd() % 6));
        else if (op == 14) pool[i] = both_full(xyzzw_identity(), pool[j], "identity + sum");
        else pool[i] = both_full(pool[j], xyzzw_identity(), "sum + identity");
    }
    for (int i = 0; i < 16; i++) if (!is_inf(pool[i])) { const FqW9 a = reduce_full(mulw(sqrw(pool[i].zz), pool[i].zz)), b = reduce_full(sqrw(pool[i].zzz)); if (!same(a, b)) { fbad++; printf("zz^3 != zzz^2 at the end of the walk\n"); } }
    printf("mixed addition: %d mismatches in %d cases (%d P = +-Q, %d from a fresh accumulator)\n", mbad, mcases, mspecial, mfresh);
    printf("full addition: %d mismatches in %d cases (%d on the hot path, %d doublings in other coordinates, %d results the identity)\n", fbad, fcases, fhot, fdbl, fident);
    printf("additions (x and y not negated) whose integers differ from the old form's (by multiples of p): %d\n", not_same_integers);
    return (bad + mbad + fbad) ? 1 : 0;
}
