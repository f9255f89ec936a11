// Host-side check of the products by a shared factor held in two forms (field29_dev.h: make_tw2_a, mul_tw2, mul_tw2_2, mul_tw2_mulw) and of the
// mixed addition of msm_accumulate's plain kernel built on them (ec29_dev.h: xyzzw_add_mixed_nflag).  Built and run by
// tests/test_field29_shared_factor_host.py with hipcc; needs no GPU.  A stand-alone program: it may also be built with
// -fsanitize=address,undefined and run directly.
//   1. The forms against mulw as residues mod p: reduce_full(tw2(z; A, w)) == reduce_full(mulw(z, w)) and A == w * 2^-116 (mulw by the limb unit
//      2^145).  Every chain is shadowed in 128 bits: no column reaches 2^64, the form returns the shadow's limbs, output limbs are normalised
//      (A: limbs 0..4 below 2^30), the lazy form's integer is the masked form's or that plus p.  The shadow taken with every operand at its declared
//      limb bound and every digit at its largest value (2^32 - 1 unmasked, 2^29 - 1 masked) must give the compile-time worst case exactly.
//      Operands: > 10^5 random ones in the shapes the addition feeds in; every limb at the declared bound (z all ones in 29 bits, A at LbTw2A's
//      limbs); w = 0, 1, p - 1; the accumulator's coordinate bounds.
//   2. The addition: chains of 250 additions, the new form beside the one it replaces (xyzzw_add_mixed_flag_impl<true, false>), each carrying
//      its own accumulator; started from accumulators at the coordinate bounds (x, y = 6p - 1, zz, zzz = 1.3p - 1), from random ones and from
//      a fresh one, with both signs of the point.  After every step: the same residues in all four coordinates, the same flag, every limb
//      below 2^29 (LbNorm, what the next addition declares for each of them), x, y < 6p and zz, zzz < 1.3p.
#include "ec29_dev.h"
#include <cstdio>
#include <cstdlib>
using namespace plk;
typedef unsigned __int128 u128;
static uint64_t rs = 0x2545f4914f6cdd1dULL;
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

// ---- 128-bit shadows.  force: every digit at its largest value instead of the one that clears the column (the compile-time worst case)
struct Shadow { u128 top; FqW9 r; bool top_limb_ok; };
static Shadow shadow_tw2(const FqW9 &z, const FqW9 &a, const FqW9 &w, unsigned lz, bool force = false) {
    Shadow s; s.top = 0; s.r = w_zero<FqW>();
    uint32_t m[5];
    u128 acc = 0;
    for (int k = 0; k < 13; k++) {
        for (int i = 0; i < 4; i++) if (k - i >= 0 && k - i <= 8) acc += (u128)z.l[i] * a.l[k - i];
        for (int i = 0; i < 5; i++) if (k - i >= 0 && k - i <= 8) acc += (u128)z.l[4 + i] * w.l[k - i];
        for (int i = 0; i < 5; i++) if (i < k && k - i <= 8) acc += (u128)m[i] * FqW::P29[k - i];
        if (k < 5) {
            const bool lazy = k < 4 && ((lz >> k) & 1u);
            m[k] = (uint32_t)acc * FqW::INV29; if (!lazy) m[k] &= M29;
            if (force) m[k] = lazy ? 0xffffffffu : M29;
            acc += (u128)m[k] * FqW::P29[0];
        }
        if (acc > s.top) s.top = acc;
        if (k >= 5) s.r.l[k - 5] = (uint32_t)acc & M29;
        acc >>= 29;
    }
    s.r.l[8] = (uint32_t)acc; s.top_limb_ok = (acc >> 32) == 0;
    return s;
}
static Shadow shadow_a(const FqW9 &w, unsigned lz, bool force = false) {
    Shadow s; s.top = 0; s.r = w_zero<FqW>();
    uint32_t m[4];
    u128 acc = 0;
    for (int k = 0; k < 12; k++) {
        if (k < 4) acc += w.l[k];
        for (int i = 0; i < 4; i++) if (i < k && k - i <= 8) acc += (u128)m[i] * FqW::P29[k - i];
        if (k < 4) {
            const bool lazy = k < 3 && ((lz >> k) & 1u);
            m[k] = (uint32_t)acc * FqW::INV29; if (!lazy) m[k] &= M29;
            if (force) m[k] = lazy ? 0xffffffffu : M29;
            acc += (u128)m[k] * FqW::P29[0];
        }
        if (acc > s.top) s.top = acc;
        if (k >= 4) s.r.l[k - 4] = (uint32_t)acc & M29;
        acc >>= 29;
    }
    s.r.l[8] = (uint32_t)acc; s.top_limb_ok = (acc >> 32) == 0;
    for (int j = 0; j < 5; j++) s.r.l[j] += w.l[4 + j];
    return s;
}

enum { F_A = 0, F_TW2 = 1, F_PAIR = 2, F_MIX = 3 };
static const char *FORM[4] = {"make_tw2_a", "mul_tw2", "mul_tw2_2", "mul_tw2_mulw"};
static int bad = 0, calls[4] = {0, 0, 0, 0}, plus_p = 0, same_int = 0;
static u128 top_seen[4] = {0, 0, 0, 0};
static void fail(const char *what, int form, const char *kind) { bad++; if (bad < 12) printf("%s: %s (%s, call %d)\n", FORM[form], what, kind, calls[form]); }
static void judge(int form, const Shadow &s, const FqW9 &got, const char *kind) {
    if (s.top > top_seen[form]) top_seen[form] = s.top;
    if (s.top >> 64) fail("a column exceeds 64 bits", form, kind);
    if (!s.top_limb_ok) fail("the top limb exceeds 32 bits", form, kind);
    if (!same(got, s.r)) fail("the form's limbs are not the shadow's", form, kind);
    for (int i = 0; i < 8; i++) if (got.l[i] > (form == F_A && i < 5 ? (1u << 30) - 1 : M29)) { fail("an output limb exceeds its bound", form, kind); break; }
}
static FqW9 E145;
// real: A is make_tw2_a(w) and the values are the addition's, so residues and value bounds are checked too
static void check_forms(const FqW9 &z0, const FqW9 &z1, const FqW9 &w, const FqW9 *a_given, const char *kind) {
    const bool real = a_given == nullptr;
    FqW9 a = real ? make_tw2_a<FqW>(w) : *a_given;
    if (real) {
        judge(F_A, shadow_a(w, TW2A_LZ_ALL), a, kind);
        const FqW9 am = make_tw2_a<FqW, 0>(w);
        judge(F_A, shadow_a(w, 0), am, kind);
        if (diff_class(normw(a), normw(am)) < 0) fail("lazy A - masked A is neither 0 nor p", F_A, kind);
        if (!same(reduce_full(normw(a)), reduce_full(mulw<FqW>(w, E145)))) fail("A is not w * 2^-116 (mod p)", F_A, kind);
        for (int i = 0; i < 9; i++) if (a.l[i] > LbTw2A::B.l[i]) fail("A exceeds LbTw2A", F_A, kind);
        calls[F_A]++;
    }
    // one chain, masked and lazy
    const FqW9 r_m = mul_tw2<FqW>(z0, a, w), r_l = mul_tw2<FqW, TW2_LZ_ALL>(z0, a, w);
    judge(F_TW2, shadow_tw2(z0, a, w, 0), r_m, kind);
    judge(F_TW2, shadow_tw2(z0, a, w, TW2_LZ_ALL), r_l, kind);
    const int d = diff_class(r_l, r_m);
    if (d < 0) fail("lazy result - masked result is neither 0 nor p", F_TW2, kind); else if (d) plus_p++; else same_int++;
    calls[F_TW2]++;
    // the lockstep pair, as the addition instantiates it
    FqW9 r0, r1;
    mul_tw2_2<FqW, TW2_LZ_ALL, TW2_LZ_ALL>(z0, a, w, z1, a, w, r0, r1);
    if (!same(r0, r_l)) fail("chain 0 is not the single chain's result", F_PAIR, kind);
    judge(F_PAIR, shadow_tw2(z1, a, w, TW2_LZ_ALL), r1, kind);
    calls[F_PAIR]++;
    // tw2 beside a plain product
    FqW9 h0, h1, o0, o1;
    mul_tw2_mulw<FqW, TW2_LZ_ALL, LZ_ALL>(z0, a, w, z1, w, h0, h1);
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm>(z1, w, z1, w, o0, o1);
    judge(F_MIX, shadow_tw2(z0, a, w, TW2_LZ_ALL), h0, kind);
    if (!same(h1, o0)) fail("the plain chain is not mulw2_lz's result", F_MIX, kind);
    calls[F_MIX]++;
    if (real) {
        if (!same(reduce_full(r_l), reduce_full(mulw<FqW>(z0, w))) || !same(reduce_full(r_m), reduce_full(mulw<FqW>(z0, w)))) fail("not mulw's residue", F_TW2, kind);
        if (!same(reduce_full(r1), reduce_full(mulw<FqW>(z1, w)))) fail("not mulw's residue", F_PAIR, kind);
        if (!same(reduce_full(h0), reduce_full(mulw<FqW>(z0, w)))) fail("not mulw's residue", F_MIX, kind);
        // z < 6.1p, w < 1.3p: below 6.1 * 1.3 * 0.0059 p + p (1 + 2^-26) + A / 2^29 < 1.05p
        static const FqW9 B105 = p_times(105, 100);
        if (!less(r_l, B105) || !less(r1, B105) || !less(h0, B105)) fail("a result is not below 1.05p", F_TW2, kind);
    }
}

static int abad = 0, adds = 0, chains = 0, afresh = 0;
static FqW9 SIX_P, P13_10;
static bool norm_limbs(const FqW9 &a) { for (int i = 0; i < 9; i++) if (a.l[i] > M29) return false; return true; }
static void run_chain(XyzzW start, bool fresh, int len, const char *what) {
    XyzzW a = start, b = start;
    bool fa = fresh, fb = fresh;
    chains++;
    for (int s = 0; s < len; s++) {
        AffW q; q.x = csub_p(rnd_w()); q.y = csub_p(rnd_w());
        const bool neg = rnd() & 1;
        afresh += fa;
        xyzzw_add_mixed_nflag(a, fa, q, neg);
        xyzzw_add_mixed_flag_impl<true, false>(b, fb, q, neg);
        adds++;
        const FqW9 *g[4] = {&a.x, &a.y, &a.zz, &a.zzz}, *w[4] = {&b.x, &b.y, &b.zz, &b.zzz};
        bool ok = fa == fb;
        for (int c = 0; c < 4; c++) ok = ok && norm_limbs(*g[c]) && same(reduce_full(*g[c]), reduce_full(*w[c]));
        ok = ok && less(a.x, SIX_P) && less(a.y, SIX_P) && less(a.zz, P13_10) && less(a.zzz, P13_10);
        if (!ok) { abad++; if (abad < 8) printf("mixed addition mismatch: %s (chain %d, step %d, neg %d)\n", what, chains, s, (int)neg); return; }
    }
}

int main() {
    SIX_P = p_times(6); P13_10 = p_times(13, 10);
    E145 = w_zero<FqW>(); E145.l[5] = 1;
    const double TWO64 = 18446744073709551616.0;
    // ---------------------------------------------------------------- 1. the forms
    const ColBound cb_a = tw2a_col_bound(LbNorm::B, FqW::P29, TW2A_LZ_ALL), cb_t = tw2_col_bound(LbNorm::B, LbTw2A::B, LbNorm::B, FqW::P29, TW2_LZ_ALL);
    // (a) every limb at its declared bound; with the digits forced to their largest values the shadow is the compile-time worst case
    {
        const FqW9 n = at(LbNorm::B), ab = at(LbTw2A::B);
        check_forms(n, n, n, &ab, "limbs at the declared bounds");
        if (shadow_tw2(n, ab, n, TW2_LZ_ALL, true).top != (u128)cb_t.worst) { bad++; printf("mul_tw2: the shadow at the bounds with the largest digits is not the compile-time worst case\n"); }
        if (shadow_a(n, TW2A_LZ_ALL, true).top != (u128)cb_a.worst) { bad++; printf("make_tw2_a: the shadow at the bounds with the largest digits is not the compile-time worst case\n"); }
        // A formed from a w with every limb at the bound (its value then is not below 2^261 / 2^116 + p, but the chain's limbs hold)
        judge(F_A, shadow_a(n, TW2A_LZ_ALL), make_tw2_a<FqW>(n), "w at the declared bound"); calls[F_A]++;
        // lower limbs at the bound under top limbs as small as the values are
        FqW9 n6 = n, n13 = n; n6.l[8] = SIX_P.l[8]; n13.l[8] = P13_10.l[8];
        check_forms(n6, n13, n13, nullptr, "lower limbs at the declared bounds");
        FqW9 a13 = make_tw2_a<FqW>(n13); for (int i = 0; i < 5; i++) a13.l[i] = (1u << 30) - 1;
        check_forms(n6, n13, n13, &a13, "A's low limbs at the declared bound");
    }
    // (b) w = 0, 1, p - 1 (as integers), z random, at the bounds and all ones
    {
        FqW9 one = w_zero<FqW>(); one.l[0] = 1;
        const FqW9 ws[4] = {w_zero<FqW>(), one, minus_one(p_times(1)), w_one<FqW>()};
        for (int j = 0; j < 4; j++) for (int it = 0; it < 50; it++) {
            FqW9 z0 = addn(rnd_w(), p_times(rnd() % 5)), z1 = rnd_w();
            if (it == 0) { z0 = minus_one(SIX_P); z1 = minus_one(P13_10); }
            if (it == 1) { z0 = at(LbNorm::B); z0.l[8] = SIX_P.l[8] - 1; z1 = z0; }
            if (it == 2) { z0 = w_zero<FqW>(); }
            check_forms(z0, z1, ws[j], nullptr, "w = 0, 1, p - 1, one");
        }
    }
    // (c) random operands in the shapes the addition feeds in: z = P (< 7.1p), -X (< 6.1p), ZZ (< 1.3p); w = PP (< 1.3p)
    for (int it = 0; it < 110000; it++) {
        FqW9 z0 = addn(rnd_w(), p_times(rnd() % 6)), z1 = rnd_w(), w = rnd_w();
        if ((it & 31) == 1) { z0 = minus_one(SIX_P); z1 = minus_one(P13_10); }
        if ((it & 31) == 2) w = minus_one(P13_10);
        if ((it & 31) == 3) { for (int i = 0; i < 8; i++) z0.l[i] = z1.l[i] = M29; z0.l[8] = SIX_P.l[8] - 1; z1.l[8] = P13_10.l[8] - 1; }
        if ((it & 31) == 4) { for (int i = 0; i < 8; i++) w.l[i] = M29; w.l[8] = P13_10.l[8] - 1; }
        if ((it & 31) == 5) w = sqrw<FqW>(z0);                 // a square, as PP is
        check_forms(z0, z1, w, nullptr, "random operands");
    }
    const u128 seen_t = top_seen[F_TW2] > top_seen[F_PAIR] ? (top_seen[F_TW2] > top_seen[F_MIX] ? top_seen[F_TW2] : top_seen[F_MIX]) : (top_seen[F_PAIR] > top_seen[F_MIX] ? top_seen[F_PAIR] : top_seen[F_MIX]);
    printf("make_tw2_a: %d calls; largest column %.6f * 2^64 (compile-time worst case %.6f * 2^64, fits: %d)\n", calls[F_A], (double)top_seen[F_A] / TWO64, (double)cb_a.worst / TWO64, (int)cb_a.fits);
    printf("mul_tw2: %d calls (%d pairs, %d beside a plain product), %d lazy results equal to the masked form's, %d larger by p; largest column %.6f * 2^64 (compile-time worst case %.6f * 2^64, fits: %d)\n",
           calls[F_TW2], calls[F_PAIR], calls[F_MIX], same_int, plus_p, (double)seen_t / TWO64, (double)cb_t.worst / TWO64, (int)cb_t.fits);
    if (!cb_a.fits || !cb_t.fits || top_seen[F_A] > (u128)cb_a.worst || seen_t > (u128)cb_t.worst) { bad++; printf("a column seen exceeds the compile-time worst case\n"); }
    printf("shared-factor forms: %d failures in %d calls\n", bad, calls[F_A] + calls[F_TW2] + calls[F_PAIR] + calls[F_MIX]);
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
    printf("mixed addition chains: %d mismatches in %d additions (%d chains of 250, %d from a fresh accumulator)\n", abad, adds, chains, afresh);
    return (bad + abad) ? 1 : 0;
}
