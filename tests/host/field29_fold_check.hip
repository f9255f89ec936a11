// Host-side check of the FOLDED Montgomery digits (field29_dev.h, "THE FOLD": the low digits of a reduction divided out by 2^-29 mod p instead of a
// Montgomery step) in the forms the mixed addition of msm_accumulate's plain kernel and the full addition of the 16-lane msm_task_reduce take
// (ec29_dev.h: xyzzw_add_mixed_nflag, xyzzw_add_pairs): mulw2_add_lz, mulw2_lz, sqrw2_lz
// and mul2addw_lz with digits 0..6 of nine folded, mul_tw2_2 and mul_tw2_mulw with digits 0..2 of five, make_tw2_a with digits 0..1 of four.  Built and
// run by tests/test_field29_fold_host.py with hipcc; needs no GPU.  A stand-alone program: it may also be built with -fsanitize=address,undefined and
// run directly.
//   1. Every folded form on more than 10^5 operands: the result is the residue mulw gives (plus the addend), its limbs are those of a 128-bit shadow of
//      the chain, no column of the shadow reaches 2^64 or exceeds the compile-time worst case printed beside it, output limbs are normalised, and the
//      folded result minus the unfolded (lazy) one is -p, 0 or p: a multiple of p, and no more than the value rule allows (both results lie less than
//      p (1 + 2^-26 + 2.15 * 2^-26) above a b / 2^261).  Operands: random ones in the shapes the addition feeds in; every limb at its DECLARED bound
//      (all limbs 2^29 - 1; +-y at PAD2's limbs; T and 2p - PPP at the 2^29-bias pads'; A at LbTw2A's; addends at LbAny - all 32 bits set - for which
//      only the shadow and the columns are checked, the value being out of range); operands built limb by limb so that the folded digits' low words
//      L are all 0, all 2^32 - 1, or alternate.
//   2. The additions: chains of 250 additions, xyzzw_add_mixed_nflag and xyzzw_add_pairs each beside the form it replaces (kept below with the
//      unfolded products), each carrying its own accumulator, from accumulators at the coordinate bounds, from random ones and from a fresh one, both
//      signs of the point.  After every step: the same residues in all four coordinates, the same flag, every limb below 2^29, x, y < 6p and
//      zz, zzz < 1.3p.
#include "ec29_dev.h"
#include <cstdio>
#include <cstdlib>
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
static bool norm_limbs(const FqW9 &a) { for (int i = 0; i < 9; i++) if (a.l[i] > M29) return false; return true; }
// a - b as integers (limbs 0..7 of both normalised): 0 -> 0, p -> 1, anything else -> -1
static int diff_class(const FqW9 &a, const FqW9 &b) {
    int64_t c = 0; bool zero = true, isp = true;
    for (int i = 0; i < 9; i++) {
        const int64_t s = (int64_t)a.l[i] - (int64_t)b.l[i] + c;
        const int64_t limb = i < 8 ? (s & (int64_t)M29) : s;
        c = i < 8 ? (s >> 29) : 0;
        if (limb != 0) zero = false;
        if (limb != (int64_t)FqW::P29[i]) isp = false;
    }
    return zero ? 0 : isp ? 1 : -1;
}
// |a - b| is 0 or p
static bool differ_by_0_or_p(const FqW9 &a, const FqW9 &b) { return diff_class(a, b) >= 0 || diff_class(b, a) >= 0; }

// ---- 128-bit shadows of the three scans with a fold set
struct Shadow { u128 top; FqW9 r; bool top_limb_ok; uint32_t low[9]; };
static int low_zero = 0, low_ones = 0;                        // folded digits whose low word L was 0 / 2^32 - 1 (not counted while operands are being built)
static bool counting = true;
static void folded_digit(Shadow &s, u128 &acc, uint32_t *m, int k, bool lazy) {
    m[k] = lazy ? (uint32_t)acc : (uint32_t)acc & M29;
    s.low[k] = m[k];
    if (lazy && counting) { low_zero += m[k] == 0; low_ones += m[k] == 0xffffffffu; }
    if (acc > s.top) s.top = acc;
    acc = lazy ? ((acc >> 32) << 3) : (acc >> 29);
}
// x: T pairs of operands (a_t, b_t); a squaring is the pair (x, x) - the same column sums
static Shadow shadow9(const FqW9 *const *x, int T, const FqW9 *addend, unsigned lz, unsigned fold) {
    Shadow s; s.top = 0; s.r = w_zero<FqW>();
    uint32_t m[9];
    u128 acc = 0;
    for (int k = 0; k < 17; k++) {
        for (int t = 0; t < T; t++) for (int i = (k < 9 ? 0 : k - 8); i <= (k < 9 ? k : 8); i++) acc += (u128)x[2 * t]->l[k - i] * x[2 * t + 1]->l[i];
        for (int i = 0; i < 9 && i < k; i++) {
            if (fold_digit(fold, i)) { if (k - i - 1 <= 8) acc += (u128)m[i] * FqW::FOLDC[k - i - 1]; }
            else if (k - i <= 8) acc += (u128)m[i] * FqW::P29[k - i];
        }
        if (k < 9) {
            const bool lazy = lazy_digit(lz, k);
            if (fold_digit(fold, k)) { folded_digit(s, acc, m, k, lazy); continue; }
            m[k] = (uint32_t)acc * FqW::INV29; if (!lazy) m[k] &= M29;
            acc += (u128)m[k] * FqW::P29[0];
        } else {
            if (addend) acc += addend->l[k - 9];
            s.r.l[k - 9] = (uint32_t)acc & M29;
        }
        if (acc > s.top) s.top = acc;
        acc >>= 29;
    }
    s.r.l[8] = (uint32_t)acc; s.top_limb_ok = (acc >> 32) == 0;
    if (addend) s.r.l[8] += addend->l[8];
    return s;
}
static Shadow shadow_tw2(const FqW9 &z, const FqW9 &a, const FqW9 &w, unsigned lz, unsigned fold) {
    Shadow s; s.top = 0; s.r = w_zero<FqW>();
    uint32_t m[5];
    u128 acc = 0;
    for (int k = 0; k < 13; k++) {
        for (int i = 0; i < 4; i++) if (k - i >= 0 && k - i <= 8) acc += (u128)z.l[i] * a.l[k - i];
        for (int i = 0; i < 5; i++) if (k - i >= 0 && k - i <= 8) acc += (u128)z.l[4 + i] * w.l[k - i];
        for (int i = 0; i < 5 && i < k; i++) {
            if (fold_digit(fold, i)) { if (k - i - 1 <= 8) acc += (u128)m[i] * FqW::FOLDC[k - i - 1]; }
            else if (k - i <= 8) acc += (u128)m[i] * FqW::P29[k - i];
        }
        if (k < 5) {
            const bool lazy = k < 4 && ((lz >> k) & 1u);
            if (fold_digit(fold, k)) { folded_digit(s, acc, m, k, lazy); continue; }
            m[k] = (uint32_t)acc * FqW::INV29; if (!lazy) m[k] &= M29;
            acc += (u128)m[k] * FqW::P29[0];
        } else s.r.l[k - 5] = (uint32_t)acc & M29;
        if (acc > s.top) s.top = acc;
        acc >>= 29;
    }
    s.r.l[8] = (uint32_t)acc; s.top_limb_ok = (acc >> 32) == 0;
    return s;
}
static Shadow shadow_a(const FqW9 &w, unsigned lz, unsigned fold) {
    Shadow s; s.top = 0; s.r = w_zero<FqW>();
    uint32_t m[4];
    u128 acc = 0;
    for (int k = 0; k < 12; k++) {
        if (k < 4) acc += w.l[k];
        for (int i = 0; i < 4 && i < k; i++) {
            if (fold_digit(fold, i)) { if (k - i - 1 <= 8) acc += (u128)m[i] * FqW::FOLDC[k - i - 1]; }
            else if (k - i <= 8) acc += (u128)m[i] * FqW::P29[k - i];
        }
        if (k < 4) {
            const bool lazy = k < 3 && ((lz >> k) & 1u);
            if (fold_digit(fold, k)) { folded_digit(s, acc, m, k, lazy); continue; }
            m[k] = (uint32_t)acc * FqW::INV29; if (!lazy) m[k] &= M29;
            acc += (u128)m[k] * FqW::P29[0];
        } else s.r.l[k - 4] = (uint32_t)acc & M29;
        if (acc > s.top) s.top = acc;
        acc >>= 29;
    }
    s.r.l[8] = (uint32_t)acc; s.top_limb_ok = (acc >> 32) == 0;
    for (int j = 0; j < 5; j++) s.r.l[j] += w.l[4 + j];
    return s;
}

enum { F_PADD = 0, F_YADD, F_PANY, F_YANY, F_SQR, F_Y3, F_A, F_TW2, F_MIXT, F_MIXM, NFORMS };
static const char *FORM[NFORMS] = {"mulw2_add_lz, normalised, addend normalised", "mulw2_add_lz, +-y, addend normalised", "mulw2_add_lz, normalised, addend LbAny",
                                   "mulw2_add_lz, +-y, addend LbAny", "sqrw2_lz", "mul2addw_lz (Y3)", "make_tw2_a", "mul_tw2_2", "mul_tw2_mulw: tw2 chain", "mul_tw2_mulw: plain chain"};
static int bad = 0, calls[NFORMS], d_zero = 0, d_p = 0;
static u128 top_seen[NFORMS];
static void fail(const char *what, int form, const char *kind) { bad++; if (bad < 16) printf("%s: %s (%s, call %d)\n", FORM[form], what, kind, calls[form]); }
static void judge(int form, const Shadow &s, const FqW9 &got, const char *kind) {
    calls[form]++;
    if (s.top > top_seen[form]) top_seen[form] = s.top;
    if (s.top >> 64) fail("a column exceeds 64 bits", form, kind);
    if (!s.top_limb_ok) fail("the top limb exceeds 32 bits", form, kind);
    if (!same(got, s.r)) fail("the form's limbs are not the shadow's", form, kind);
    for (int i = 0; i < 8; i++) if (got.l[i] > (form == F_A && i < 5 ? (1u << 30) - 1 : M29)) { fail("an output limb exceeds its bound", form, kind); break; }
}
// folded beside unfolded: the same residue, and integers that differ by 0 or p
static void beside(int form, const FqW9 &folded, const FqW9 &unfolded, const FqW9 *want, const char *kind) {
    const FqW9 f = form == F_A ? normw(folded) : folded, u = form == F_A ? normw(unfolded) : unfolded;
    if (!differ_by_0_or_p(f, u)) fail("folded result - unfolded result is not -p, 0 or p", form, kind);
    else if (same(f, u)) d_zero++; else d_p++;
    if (want && !same(reduce_full(f), *want)) fail("not the residue mulw gives", form, kind);
}
static FqW9 E145;
// the product pair with addends, P = U2 + NX and R = S2 + NY: (xq, zz, ax), (yq, zzz, ay).  real: values in range, residues checked too
template <class LAD>
static void check_padd(const FqW9 &xq, const FqW9 &zz, const FqW9 &ax, const FqW9 &yq, const FqW9 &zzz, const FqW9 &ay, bool real, const char *kind) {
    constexpr bool ANY = std::is_same<LAD, LbAny>::value;
    FqW9 p, r, pu, ru;
    mulw2_add_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LAD, LbSignedY, LbNorm, LAD, FOLD9>(xq, zz, ax, yq, zzz, ay, p, r);
    mulw2_add_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LAD, LbSignedY, LbNorm, LAD>(xq, zz, ax, yq, zzz, ay, pu, ru);
    const FqW9 *x0[2] = {&xq, &zz}, *x1[2] = {&yq, &zzz};
    judge(ANY ? F_PANY : F_PADD, shadow9(x0, 1, &ax, LZ_ALL, FOLD9), p, kind);
    judge(ANY ? F_YANY : F_YADD, shadow9(x1, 1, &ay, LZ_ALL, FOLD9), r, kind);
    if (!real) return;
    const FqW9 wp = reduce_full(addn(mulw<FqW>(xq, zz), normw(ax))), wr = reduce_full(addn(mulw<FqW>(yq, zzz), normw(ay)));
    beside(ANY ? F_PANY : F_PADD, p, pu, &wp, kind);
    beside(ANY ? F_YANY : F_YADD, r, ru, &wr, kind);
}
static void check_sqr(const FqW9 &p, const FqW9 &r, bool real, const char *kind) {
    FqW9 pp, rr, ppu, rru;
    sqrw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, FOLD9>(p, r, pp, rr);
    sqrw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm>(p, r, ppu, rru);
    const FqW9 *x0[2] = {&p, &p}, *x1[2] = {&r, &r};
    judge(F_SQR, shadow9(x0, 1, nullptr, LZ_ALL, FOLD9), pp, kind);
    judge(F_SQR, shadow9(x1, 1, nullptr, LZ_ALL, FOLD9), rr, kind);
    if (!real) return;
    const FqW9 w0 = reduce_full(mulw<FqW>(p, p)), w1 = reduce_full(mulw<FqW>(r, r));
    beside(F_SQR, pp, ppu, &w0, kind);
    beside(F_SQR, rr, rru, &w1, kind);
}
// the fused Y3 = r * t + y * nppp
static void check_y3(const FqW9 &r, const FqW9 &t, const FqW9 &y, const FqW9 &nppp, bool real, const char *kind) {
    const FqW9 got = WMA_LZF(r, t, y, nppp, FOLD9), unf = WMA_LZ(r, t, y, nppp);
    const FqW9 *x[4] = {&r, &t, &y, &nppp};
    judge(F_Y3, shadow9(x, 2, nullptr, LZ_ALL, FOLD9), got, kind);
    if (!real) return;
    const FqW9 want = reduce_full(addn(mulw<FqW>(t, r), mulw<FqW>(nppp, y)));
    beside(F_Y3, got, unf, &want, kind);
}
// the shared factor: A, the pair (PPP, NQ), ZZ3 beside the plain ZZZ3 = x * y
static void check_tw2(const FqW9 &z0, const FqW9 &z1, const FqW9 &w, const FqW9 *a_given, const FqW9 &x, const FqW9 &y, const char *kind) {
    const bool real = a_given == nullptr;
    FqW9 a = real ? make_tw2_a<FqW, TW2A_LZ_ALL, LbNorm, FOLD_TW2A>(w) : *a_given;
    if (real) {
        judge(F_A, shadow_a(w, TW2A_LZ_ALL, FOLD_TW2A), a, kind);
        const FqW9 want = reduce_full(mulw<FqW>(w, E145));
        beside(F_A, a, make_tw2_a<FqW>(w), &want, kind);
        for (int i = 0; i < 9; i++) if (a.l[i] > LbTw2A::B.l[i]) fail("A exceeds LbTw2A", F_A, kind);
    }
    FqW9 r0, r1, u0, u1, h0, h1, g0, g1;
    mul_tw2_2<FqW, TW2_LZ_ALL, TW2_LZ_ALL, LbNorm, LbNorm, LbTw2A, LbNorm, FOLD_TW2>(z0, a, w, z1, a, w, r0, r1);
    mul_tw2_2<FqW, TW2_LZ_ALL, TW2_LZ_ALL>(z0, a, w, z1, a, w, u0, u1);
    judge(F_TW2, shadow_tw2(z0, a, w, TW2_LZ_ALL, FOLD_TW2), r0, kind);
    judge(F_TW2, shadow_tw2(z1, a, w, TW2_LZ_ALL, FOLD_TW2), r1, kind);
    mul_tw2_mulw<FqW, TW2_LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbTw2A, LbNorm, FOLD_TW2, FOLD9>(z0, a, w, x, y, h0, h1);
    mul_tw2_mulw<FqW, TW2_LZ_ALL, LZ_ALL>(z0, a, w, x, y, g0, g1);
    const FqW9 *xy[2] = {&x, &y};
    judge(F_MIXT, shadow_tw2(z0, a, w, TW2_LZ_ALL, FOLD_TW2), h0, kind);
    judge(F_MIXM, shadow9(xy, 1, nullptr, LZ_ALL, FOLD9), h1, kind);
    if (!real) return;
    const FqW9 w0 = reduce_full(mulw<FqW>(z0, w)), w1 = reduce_full(mulw<FqW>(z1, w)), w2 = reduce_full(mulw<FqW>(x, y));
    beside(F_TW2, r0, u0, &w0, kind);
    beside(F_TW2, r1, u1, &w1, kind);
    beside(F_MIXT, h0, g0, &w0, kind);
    beside(F_MIXM, h1, g1, &w2, kind);
    // z < 7.1p, w, x, y < 1.3p: below 7.1 * 1.3 * 0.0059 p + p (1 + 2^-26) + A / 2^29 + 2.15 * 2^-26 p < 1.06p
    static const FqW9 B106 = p_times(106, 100);
    if (!less(r0, B106) || !less(r1, B106) || !less(h0, B106) || !less(h1, B106)) fail("a result is not below 1.06p", F_TW2, kind);
}

// operands a, b (normalised) of a plain folded product whose folded digits' low words are want[k]: limb k of b at random, limb k of a solved from
// column k (a_k b_0 + the rest = want mod 2^32; b_0 odd), tried until it is below 2^29
static bool build_low_words(const uint32_t want[7], FqW9 &a, FqW9 &b) {
    a = w_zero<FqW>(); b = w_zero<FqW>();
    b.l[0] = (rnd() & M29) | 1u;
    uint32_t inv = b.l[0];                                     // b_0^-1 mod 2^32 (Newton)
    for (int i = 0; i < 5; i++) inv *= 2u - b.l[0] * inv;
    const FqW9 *x[2] = {&a, &b};
    for (int k = 0; k < 7; k++) {
        int tries = 0;
        for (;; tries++) {
            if (tries > 2000) return false;
            if (k > 0) b.l[k] = rnd() & M29;
            a.l[k] = 0;
            const uint32_t rest = shadow9(x, 1, nullptr, LZ_ALL, FOLD9).low[k];
            a.l[k] = (want[k] - rest) * inv;
            if (a.l[k] <= M29) break;
        }
    }
    a.l[7] = rnd() & M29; b.l[7] = rnd() & M29; a.l[8] = rnd() & 0x3fffff; b.l[8] = rnd() & 0x3fffff;   // < 2^254: a product below 1.1p
    return true;
}

// ---- the mixed addition as it was before the fold (the text of xyzzw_add_mixed_flag_impl<true, true> with every product unfolded)
static void unfolded_add_mixed_nflag(XyzzW &acc, bool &fresh, const AffW &q, bool neg_q) {
    if (fresh) { acc.x = neg2(q.x); acc.y = neg_q ? q.y : neg2(q.y); acc.zz = w_one<FqW>(); acc.zzz = w_one<FqW>(); fresh = false; return; }
    FqW9 p, r, yq;
    for (int i = 0; i < 9; i++) yq.l[i] = neg_q ? FqW::PAD2[i] - q.y.l[i] : q.y.l[i];
    mulw2_add_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbSignedY, LbNorm, LbNorm>(q.x, acc.zz, acc.x, yq, acc.zzz, acc.y, p, r);
    if (maybe_zero_mod_p(p)) {
        AffW t; t.x = q.x; t.y = normw(yq);
        acc = xyzzw_flip_xy(acc);
        xyzzw_add_mixed_special(acc, t, false, p, r);
        fresh = is_inf(acc);
        acc = xyzzw_flip_xy(acc);
        return;
    }
    FqW9 pp, rr, ppp, qq;
    sqrw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm>(p, r, pp, rr);
    const FqW9 a_pp = make_tw2_a<FqW>(pp);
    mul_tw2_2<FqW, TW2_LZ_ALL, TW2_LZ_ALL>(p, a_pp, pp, acc.x, a_pp, pp, ppp, qq);
    FqW9 x3;
    for (int i = 0; i < 9; i++) x3.l[i] = ppp.l[i] + FqW::PAD4[i] - rr.l[i] - 2 * qq.l[i];
    x3 = normw(x3);
    FqW9 zz3, zzz3;
    mul_tw2_mulw<FqW, TW2_LZ_ALL, LZ_ALL>(acc.zz, a_pp, pp, acc.zzz, ppp, zz3, zzz3);
    FqW9 t, nppp;
    for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; nppp.l[i] = FqW::PAD2N[i] - ppp.l[i]; }
    acc.y = WMA_LZ(r, t, acc.y, nppp);
    acc.x = x3; acc.zz = zz3; acc.zzz = zzz3;
}
static int abad = 0, adds = 0, chains = 0, afresh = 0, aints = 0;
static FqW9 SIX_P, P13_10;
static void run_chain(XyzzW start, bool fresh, int len, const char *what) {
    XyzzW a = start, b = start;
    bool fa = fresh, fb = fresh;
    chains++;
    for (int s = 0; s < len; s++) {
        AffW q; q.x = csub_p(rnd_w()); q.y = csub_p(rnd_w());
        const bool neg = rnd() & 1;
        afresh += fa;
        xyzzw_add_mixed_nflag(a, fa, q, neg);
        unfolded_add_mixed_nflag(b, fb, q, neg);
        adds++;
        const FqW9 *g[4] = {&a.x, &a.y, &a.zz, &a.zzz}, *w[4] = {&b.x, &b.y, &b.zz, &b.zzz};
        bool ok = fa == fb, ints = true;
        for (int c = 0; c < 4; c++) { ok = ok && norm_limbs(*g[c]) && same(reduce_full(*g[c]), reduce_full(*w[c])); ints = ints && same(*g[c], *w[c]); }
        aints += ints;
        ok = ok && less(a.x, SIX_P) && less(a.y, SIX_P) && less(a.zz, P13_10) && less(a.zzz, P13_10);
        if (!ok) { abad++; if (abad < 8) printf("mixed addition mismatch: %s (chain %d, step %d, neg %d)\n", what, chains, s, (int)neg); return; }
    }
}

// ---- the full addition of the 16-lane reduction as it was before the fold (the hot path of xyzzw_add_pairs with every product unfolded)
static void unfolded_add_pairs(XyzzW &a, const XyzzW &b) {
    if (is_inf(b)) return;
    if (is_inf(a)) { a = b; return; }
    FqW9 u1, s1, p, r, nu, ns;
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm>(a.x, b.zz, a.y, b.zzz, u1, s1);
    for (int i = 0; i < 9; i++) { nu.l[i] = FqW::PAD2[i] - u1.l[i]; ns.l[i] = FqW::PAD2[i] - s1.l[i]; }
    mulw2_add_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbAny, LbNorm, LbNorm, LbAny>(b.x, a.zz, nu, b.y, a.zzz, ns, p, r);
    if (is_zero_mod_p(p)) { if (is_zero_mod_p(r)) a = xyzzw_double(a); else a = xyzzw_identity(); return; }
    FqW9 zz12, zzz12, pp, rr, ppp, qq, x3, t, nppp;
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm>(a.zz, b.zz, a.zzz, b.zzz, zz12, zzz12);
    sqrw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm>(p, r, pp, rr);
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm>(p, pp, u1, pp, ppp, qq);
    for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
    x3 = normw(x3);
    for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; nppp.l[i] = FqW::PAD2N[i] - ppp.l[i]; }
    a.y = WMA_LZ(r, t, s1, nppp);
    a.x = x3;
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm>(zz12, pp, zzz12, ppp, a.zz, a.zzz);
}
static int pbad = 0, padds = 0, pchains = 0, pints = 0;
static XyzzW rnd_xyzz() { XyzzW s; s.x = addn(rnd_w(), p_times(rnd() % 5)); s.y = addn(rnd_w(), p_times(rnd() % 5)); s.zz = rnd_w(); s.zzz = rnd_w(); return s; }
static void run_pairs_chain(XyzzW start, const XyzzW *fixed, int len, const char *what) {
    XyzzW a = start, b = start;
    pchains++;
    for (int s = 0; s < len; s++) {
        const XyzzW q = fixed && (s & 1) ? *fixed : rnd_xyzz();
        xyzzw_add_pairs(a, q);
        unfolded_add_pairs(b, q);
        padds++;
        const FqW9 *g[4] = {&a.x, &a.y, &a.zz, &a.zzz}, *w[4] = {&b.x, &b.y, &b.zz, &b.zzz};
        bool ok = is_inf(a) == is_inf(b), ints = true;
        for (int c = 0; c < 4; c++) { ok = ok && norm_limbs(*g[c]) && same(reduce_full(*g[c]), reduce_full(*w[c])); ints = ints && same(*g[c], *w[c]); }
        pints += ints;
        ok = ok && less(a.x, SIX_P) && less(a.y, SIX_P) && less(a.zz, P13_10) && less(a.zzz, P13_10);
        if (!ok) { pbad++; if (pbad < 8) printf("full addition mismatch: %s (chain %d, step %d)\n", what, pchains, s); return; }
    }
}

int main() {
    SIX_P = p_times(6); P13_10 = p_times(13, 10);
    E145 = w_zero<FqW>(); E145.l[5] = 1;
    const double TWO64 = 18446744073709551616.0;
    const Limbs9 FC = lb_of(FqW::FOLDC);
    // compile-time worst cases of the instantiations, as their static_asserts evaluate them
    const ColBound cb[NFORMS] = {
        lazy_col_bound(LbNorm::B, LbNorm::B, LbNone::B, LbNone::B, LbNorm::B, FqW::P29, LZ_ALL, LbNone::B, LbNone::B, FOLD9, FC),
        lazy_col_bound(LbSignedY::B, LbNorm::B, LbNone::B, LbNone::B, LbNorm::B, FqW::P29, LZ_ALL, LbNone::B, LbNone::B, FOLD9, FC),
        lazy_col_bound(LbNorm::B, LbNorm::B, LbNone::B, LbNone::B, LbAny::B, FqW::P29, LZ_ALL, LbNone::B, LbNone::B, FOLD9, FC),
        lazy_col_bound(LbSignedY::B, LbNorm::B, LbNone::B, LbNone::B, LbAny::B, FqW::P29, LZ_ALL, LbNone::B, LbNone::B, FOLD9, FC),
        lazy_col_bound(LbNorm::B, LbNorm::B, LbNone::B, LbNone::B, LbNone::B, FqW::P29, LZ_ALL, LbNone::B, LbNone::B, FOLD9, FC),
        lazy_col_bound(LbNorm::B, LbT::B, LbNorm::B, LbNppp::B, LbNone::B, FqW::P29, LZ_ALL, LbNone::B, LbNone::B, FOLD9, FC),
        tw2a_col_bound(LbNorm::B, FqW::P29, TW2A_LZ_ALL, FOLD_TW2A, FC),
        tw2_col_bound(LbNorm::B, LbTw2A::B, LbNorm::B, FqW::P29, TW2_LZ_ALL, FOLD_TW2, FC),
        tw2_col_bound(LbNorm::B, LbTw2A::B, LbNorm::B, FqW::P29, TW2_LZ_ALL, FOLD_TW2, FC),
        lazy_col_bound(LbNorm::B, LbNorm::B, LbNone::B, LbNone::B, LbNone::B, FqW::P29, LZ_ALL, LbNone::B, LbNone::B, FOLD9, FC)};
    // ---------------------------------------------------------------- 1. the forms
    // (a) every limb at its declared bound (values out of range: shadow and columns only)
    {
        const FqW9 n = at(LbNorm::B), sy = at(LbSignedY::B), any = at(LbAny::B), t = at(LbT::B), np = at(LbNppp::B), ab = at(LbTw2A::B);
        check_padd<LbNorm>(n, n, n, sy, n, n, false, "limbs at the declared bounds");
        check_padd<LbAny>(n, n, any, sy, n, any, false, "limbs at the declared bounds");
        check_sqr(n, n, false, "limbs at the declared bounds");
        check_y3(n, t, n, np, false, "limbs at the declared bounds");
        check_tw2(n, n, n, &ab, n, n, "limbs at the declared bounds");
        judge(F_A, shadow_a(n, TW2A_LZ_ALL, FOLD_TW2A), make_tw2_a<FqW, TW2A_LZ_ALL, LbNorm, FOLD_TW2A>(n), "w at the declared bound");
        // lower limbs at the bound under top limbs as small as the values are: in range, so residues too
        FqW9 n6 = n, n13 = n, y2 = sy, t7 = t, np2 = np; n6.l[8] = SIX_P.l[8] - 1; n13.l[8] = P13_10.l[8] - 1;
        check_padd<LbNorm>(n13, n13, n6, y2, n13, n6, true, "lower limbs at the declared bounds");
        check_padd<LbAny>(n13, n13, n6, y2, n13, n6, true, "lower limbs at the declared bounds");
        check_sqr(n6, n6, true, "lower limbs at the declared bounds");
        check_y3(n6, t7, n6, np2, true, "lower limbs at the declared bounds");
        check_tw2(n6, n13, n13, nullptr, n13, n13, "lower limbs at the declared bounds");
    }
    // (b) the folded digits' low words chosen: all 0, all 2^32 - 1, alternating, one of each beside random ones
    int built = 0;
    for (int it = 0; it < 400; it++) {
        uint32_t want[7];
        for (int k = 0; k < 7; k++) {
            const int mode = it & 3;
            want[k] = mode == 0 ? 0u : mode == 1 ? 0xffffffffu : mode == 2 ? ((k & 1) ? 0xffffffffu : 0u) : (k == it % 7 ? 0u : k == (it + 3) % 7 ? 0xffffffffu : rnd());
        }
        FqW9 a, b;
        counting = false;
        const bool ok = build_low_words(want, a, b);
        counting = true;
        if (!ok) continue;
        built++;
        const FqW9 *x[2] = {&a, &b};
        const Shadow s = shadow9(x, 1, nullptr, LZ_ALL, FOLD9);
        for (int k = 0; k < 7; k++) if (s.low[k] != want[k]) fail("the built operands do not give the low words asked for", F_MIXM, "chosen low words");
        const FqW9 zero = w_zero<FqW>();
        check_padd<LbNorm>(a, b, zero, a, b, zero, true, "chosen low words");
        check_tw2(rnd_w(), rnd_w(), rnd_w(), nullptr, a, b, "chosen low words");
    }
    const int low_zero_built = low_zero, low_ones_built = low_ones;
    // low limbs of zero: every column is empty, L = 0 in every folded digit of every form
    {
        FqW9 hi = w_zero<FqW>(); hi.l[8] = 0x1000; const FqW9 zero = w_zero<FqW>();
        check_padd<LbNorm>(hi, hi, zero, hi, hi, zero, true, "low limbs zero");
        check_sqr(hi, zero, true, "low limbs zero");
        check_y3(hi, hi, zero, zero, true, "low limbs zero");
        check_tw2(zero, hi, hi, nullptr, zero, hi, "low limbs zero");
    }
    // (c) random operands in the shapes the addition feeds in
    for (int it = 0; it < 30000; it++) {
        const FqW9 xq = csub_p(rnd_w()), yqn = csub_p(rnd_w());
        const bool neg = rnd() & 1;
        FqW9 yq; for (int i = 0; i < 9; i++) yq.l[i] = neg ? FqW::PAD2[i] - yqn.l[i] : yqn.l[i];
        FqW9 nx = addn(rnd_w(), p_times(rnd() % 6)), ny = addn(rnd_w(), p_times(rnd() % 6)), zz = rnd_w(), zzz = rnd_w();
        if ((it & 31) == 1) { nx = minus_one(SIX_P); ny = minus_one(SIX_P); zz = minus_one(P13_10); zzz = minus_one(P13_10); }
        if ((it & 31) == 2) { for (int i = 0; i < 8; i++) nx.l[i] = ny.l[i] = zz.l[i] = zzz.l[i] = M29; nx.l[8] = ny.l[8] = SIX_P.l[8] - 1; zz.l[8] = zzz.l[8] = P13_10.l[8] - 1; }
        check_padd<LbNorm>(xq, zz, nx, yq, zzz, ny, true, "random operands");
        FqW9 ax, ay; for (int i = 0; i < 9; i++) { ax.l[i] = FqW::PAD6[i] - nx.l[i]; ay.l[i] = FqW::PAD8[i] - ny.l[i]; }          // padded differences as they stand
        check_padd<LbAny>(xq, zz, ax, yq, zzz, ay, true, "random operands, padded addends");
        const FqW9 p = addn(rnd_w(), p_times(rnd() % 7)), r = addn(rnd_w(), p_times(rnd() % 9));
        check_sqr(p, r, true, "random operands");
        const FqW9 qq = rnd_w(), x3 = addn(rnd_w(), p_times(rnd() % 5)), ppp = rnd_w();
        FqW9 t, nppp; for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; nppp.l[i] = FqW::PAD2N[i] - ppp.l[i]; }
        check_y3(r, t, ny, nppp, true, "random operands");
        FqW9 w = (it & 7) == 5 ? sqrw<FqW>(p) : rnd_w();
        if ((it & 31) == 4) { for (int i = 0; i < 8; i++) w.l[i] = M29; w.l[8] = P13_10.l[8] - 1; }
        check_tw2(p, nx, w, nullptr, zzz, ppp, "random operands");
    }
    int total = 0;
    for (int f = 0; f < NFORMS; f++) {
        total += calls[f];
        printf("%s: %d chains; largest column %.6f * 2^64 (compile-time worst case %.6f * 2^64, fits: %d)\n", FORM[f], calls[f], (double)top_seen[f] / TWO64, (double)cb[f].worst / TWO64, (int)cb[f].fits);
        if (!cb[f].fits || top_seen[f] > (u128)cb[f].worst) { bad++; printf("%s: a column seen exceeds the compile-time worst case\n", FORM[f]); }
    }
    printf("chosen low words: %d operand pairs built; folded digits with L = 0: %d, with L = 2^32 - 1: %d (all forms: %d, %d)\n", built, low_zero_built, low_ones_built, low_zero, low_ones);
    printf("folded beside unfolded: %d equal integers, %d differing by p\n", d_zero, d_p);
    printf("folded forms: %d failures in %d chains\n", bad, total);
    // ---------------------------------------------------------------- 2. the addition
    XyzzW top; top.x = minus_one(SIX_P); top.y = minus_one(SIX_P); top.zz = minus_one(P13_10); top.zzz = minus_one(P13_10);
    XyzzW ones; for (int i = 0; i < 8; i++) ones.x.l[i] = ones.y.l[i] = ones.zz.l[i] = ones.zzz.l[i] = M29;
    ones.x.l[8] = ones.y.l[8] = SIX_P.l[8] - 1; ones.zz.l[8] = ones.zzz.l[8] = P13_10.l[8] - 1;
    for (int c = 0; c < 40; c++) { run_chain(top, false, 250, "from the coordinate bounds"); run_chain(ones, false, 250, "from all-ones limbs under the bounds' top limbs"); }
    for (int c = 0; c < 40; c++) run_chain(xyzzw_identity(), true, 250, "from a fresh accumulator");
    for (int c = 0; c < 300; c++) {
        XyzzW s; s.x = addn(rnd_w(), p_times(rnd() % 5)); s.y = addn(rnd_w(), p_times(rnd() % 5)); s.zz = rnd_w(); s.zzz = rnd_w();
        run_chain(s, false, 250, "from a random accumulator");
    }
    printf("mixed addition chains: %d mismatches in %d additions (%d chains of 250, %d from a fresh accumulator; %d steps with the unfolded form's integers)\n", abad, adds, chains, afresh, aints);
    for (int c = 0; c < 40; c++) { run_pairs_chain(top, &top, 250, "from and with the coordinate bounds"); run_pairs_chain(ones, &ones, 250, "from and with all-ones limbs under the bounds' top limbs"); }
    for (int c = 0; c < 40; c++) run_pairs_chain(xyzzw_identity(), nullptr, 250, "from the identity");
    for (int c = 0; c < 300; c++) run_pairs_chain(rnd_xyzz(), nullptr, 250, "from a random accumulator");
    printf("full addition chains: %d mismatches in %d additions (%d chains of 250; %d steps with the unfolded form's integers)\n", pbad, padds, pchains, pints);
    return (bad + abad + pbad) ? 1 : 0;
}
