// Host-side check of the work-priced forms of the kernels around msm_accumulate against the forms they stand in for.
// Built and run by tests/test_field29_pairs_host.py with hipcc; needs no GPU.  A stand-alone program: it may also be built with
// -Xarch_host -fsanitize=address,undefined and run directly.
//   1. xyzzw_add_pairs (ec29_dev.h: the full addition of the work-bound msm_task_reduce, lockstep product-scanning pairs) == xyzzw_add in all
//      36 limbs: > 10^5 pairs of lazily reduced operands as the bucket reduction feeds them in — outputs of xyzzw_add_mixed_flag, sums of them,
//      sums of sums, doublings; coordinates at 6p / 1.3p with every lower limb at 2^29 - 1; a or b the identity, a = b (in the same and in
//      different coordinates: the doubling branch), a = -b.  Every column chain of the addition is shadowed in 128 bits at exactly the limbs
//      it is given: none reaches 0.8 * 2^64.
//   2. fr_canonical_w (field29_dev.h) == to_canonical, as integers, and recode17_w (msm_shape.h) == recode17 digit for digit: edge scalars
//      (0, 1, r - 1 and their Montgomery forms; 2^k and 2^k - 1 for every k < 254; every window at 2^16 - 1, 2^16, 2^16 + 1 — the carry
//      chain —; only the top window set), each both as the canonical value and as the input, and > 10^5 random residues and raw 256-bit words.
#include "msm_shape.h"
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
static bool same(const XyzzW &a, const XyzzW &b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.zz, b.zz) && same(a.zzz, b.zzz); }
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
// the largest normalised value below `bound` in every limb: lower limbs at 2^29 - 1, the top limb one below the bound's
static FqW9 limbs_at_max(const FqW9 &bound) { FqW9 r; for (int i = 0; i < 8; i++) r.l[i] = M29; r.l[8] = bound.l[8] - 1; return r; }

// ---- 128-bit shadows of the column chains: the largest value the 64-bit accumulator has to hold
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
static u128 shadow_sqrw(const FqW9 &x) {
    uint32_t m[9]; u128 acc = 0, top = 0;
    for (int k = 0; k < 17; k++) {
        for (int i = (k < 9 ? 0 : k - 8); 2 * i < k; i++) acc += (u128)(uint32_t)(x.l[k - i] << 1) * x.l[i];
        if (k % 2 == 0) acc += (u128)x.l[k / 2] * x.l[k / 2];
        for (int i = (k < 9 ? 0 : k - 8); i <= (k < 9 ? k - 1 : 8); i++) acc += (u128)m[i] * FqW::P29[k - i];
        if (k < 9) { m[k] = ((uint32_t)acc * FqW::INV29) & M29; acc += (u128)m[k] * FqW::P29[0]; }
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
static u128 umax(u128 a, u128 b) { return a > b ? a : b; }
static bool limbs_ok = true;                                   // every left operand below MULW_A_LIMB_MAX, every right operand and doubled limb as documented
static void left(const FqW9 &a) { for (int i = 0; i < 9; i++) if (a.l[i] > MULW_A_LIMB_MAX) limbs_ok = false; }
static void norm(const FqW9 &a) { for (int i = 0; i < 9; i++) if (a.l[i] > M29) limbs_ok = false; }
// the hot path of xyzzw_add_pairs once more, product by product with the operands it forms, every chain shadowed; also the intermediate
// differences against the helpers of xyzzw_add (sub2, sub6, neg2)
static u128 shadow_pairs(const XyzzW &a, const XyzzW &b, bool &hot) {
    const FqW9 Z = w_zero<FqW>();
    u128 top = 0;
    hot = false;
    if (is_inf(a) || is_inf(b)) return 0;
    FqW9 u1, s1, p, r, nu, ns;
    mulw2<FqW>(a.x, b.zz, a.y, b.zzz, u1, s1);
    left(a.x); left(a.y); norm(b.zz); norm(b.zzz);
    top = umax(top, umax(shadow_mulw_add(a.x, b.zz, Z), shadow_mulw_add(a.y, b.zzz, Z)));
    for (int i = 0; i < 9; i++) { nu.l[i] = FqW::PAD2[i] - u1.l[i]; ns.l[i] = FqW::PAD2[i] - s1.l[i]; if (u1.l[i] > FqW::PAD2[i] || s1.l[i] > FqW::PAD2[i]) limbs_ok = false; }
    mulw2_add<FqW>(b.x, a.zz, nu, b.y, a.zzz, ns, p, r);
    left(b.x); left(b.y); norm(a.zz); norm(a.zzz);
    top = umax(top, umax(shadow_mulw_add(b.x, a.zz, nu), shadow_mulw_add(b.y, a.zzz, ns)));
    if (!same(p, sub2(mulw(b.x, a.zz), u1)) || !same(r, sub2(mulw(b.y, a.zzz), s1))) limbs_ok = false;     // P, R as xyzzw_add forms them
    if (is_zero_mod_p(p)) return top;
    hot = true;
    FqW9 zz12, zzz12, pp, rr, ppp, qq, x3, t, nppp;
    mulw2<FqW>(a.zz, b.zz, a.zzz, b.zzz, zz12, zzz12);
    top = umax(top, umax(shadow_mulw_add(a.zz, b.zz, Z), shadow_mulw_add(a.zzz, b.zzz, Z)));
    sqrw2<FqW>(p, r, pp, rr);
    norm(p); norm(r);
    top = umax(top, umax(shadow_sqrw(p), shadow_sqrw(r)));
    mulw2<FqW>(p, pp, u1, pp, ppp, qq);
    norm(pp); norm(u1);
    top = umax(top, umax(shadow_mulw_add(p, pp, Z), shadow_mulw_add(u1, pp, Z)));
    for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
    x3 = normw(x3);
    for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; nppp.l[i] = FqW::PAD2N[i] - ppp.l[i]; if (t.l[i] > 1450000000u || nppp.l[i] > 1020000000u) limbs_ok = false; }
    if (!same(normw(t), sub6(qq, x3)) || !same(normw(nppp), neg2(ppp))) limbs_ok = false;
    norm(r); norm(s1);
    top = umax(top, shadow_mul2addw(r, t, s1, nppp));
    norm(zz12); norm(zzz12); norm(ppp);
    top = umax(top, umax(shadow_mulw_add(zz12, pp, Z), shadow_mulw_add(zzz12, ppp, Z)));
    return top;
}

static G1Affine to_aff(const G1Xyzz &p) {
    G1Affine a; if (is_inf(p)) { a.x = Fq::zero(); a.y = Fq::zero(); return a; }
    Fq i = inv(mul(p.zz, p.zzz)); a.x = mul(p.x, mul(i, p.zzz)); a.y = mul(p.y, mul(i, p.zz)); return a; }
static AffW aff_to_w(const G1Affine &a) { AffW r; r.x = csub_p(w_from_s(unpack<FqW>(a.x))); r.y = csub_p(w_from_s(unpack<FqW>(a.y))); return r; }

static int abad = 0, acases = 0, ahot = 0, adbl = 0, aid = 0;
static u128 atop = 0;
static FqW9 SIX_P, P13_10;
// a + b by both forms; returns the sum
static XyzzW both(const XyzzW &a, const XyzzW &b, const char *what) {
    XyzzW want = a, got = a;
    xyzzw_add(want, b);
    xyzzw_add_pairs(got, b);
    bool hot;
    const u128 top = shadow_pairs(a, b, hot);
    if (top > atop) atop = top;
    acases++; ahot += hot;
    bool ok = same(got, want) && top < (((u128)1 << 64) / 5) * 4;
    const FqW9 *g[4] = {&got.x, &got.y, &got.zz, &got.zzz};
    for (int c = 0; c < 4; c++) for (int i = 0; i < 8; i++) if (g[c]->l[i] > M29) ok = false;          // normalised
    if (!ok) { abad++; if (abad < 8) printf("full addition mismatch: %s (case %d)\n", what, acases); }
    return got;
}

// ---- scalars
static const uint32_t R_WORDS[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
static int sbad = 0, scases = 0;
static bool below_r(const Fr &a) { for (int i = 7; i >= 0; i--) if (a.l[i] != R_WORDS[i]) return a.l[i] < R_WORDS[i]; return false; }
static void check_input(const Fr &k, const char *what) {
    const Fr want = to_canonical(k);
    const FrW9 got = fr_canonical_w(k);
    bool ok = true;
    for (int i = 0; i < 8; i++) if (got.l[i] > M29) ok = false;
    const FrW9 w = unpack<FrW>(want);
    for (int i = 0; i < 9; i++) if (got.l[i] != w.l[i]) ok = false;
    const Fr back = pack<FrParams>(got);
    for (int i = 0; i < 8; i++) if (back.l[i] != want.l[i]) ok = false;
    int32_t d0[RC_WINDOWS], d1[RC_WINDOWS];
    recode17(want, d0);
    recode17_w(got, d1);
    for (int i = 0; i < RC_WINDOWS; i++) if (d0[i] != d1[i]) ok = false;
    scases++;
    if (!ok) { sbad++; if (sbad < 8) printf("scalar mismatch: %s (case %d)\n", what, scases); }
}
// a canonical value c: as the input itself, and as the value the input stands for (input = c * 2^256)
static void check_value(const Fr &c, const char *what) {
    check_input(c, what);
    if (!below_r(c)) return;
    const Fr mont = from_canonical(c), back = to_canonical(mont);
    for (int i = 0; i < 8; i++) if (back.l[i] != c.l[i]) { sbad++; printf("from_canonical / to_canonical do not round-trip: %s\n", what); return; }
    check_input(mont, what);
}
static Fr fr_zero() { Fr a; for (int i = 0; i < 8; i++) a.l[i] = 0; return a; }
static Fr pow2(int k) { Fr a = fr_zero(); a.l[k >> 5] = 1u << (k & 31); return a; }
static Fr pow2m1(int k) { Fr a = fr_zero(); for (int i = 0; i < k; i++) a.l[i >> 5] |= 1u << (i & 31); return a; }
static Fr windows(uint32_t v, uint32_t top) {                  // windows 0..13 = v, window 14 = top
    uint64_t w[5] = {0, 0, 0, 0, 0};                           // 64-bit words, one to spare
    for (int i = 0; i < 15; i++) {
        const uint64_t x = i < 14 ? v : top; const int pos = 17 * i;
        w[pos >> 6] += x << (pos & 63);                        // (adjacent windows never overlap below 2^17, so += is |=; v = 2^17 - 1 at most)
        if ((pos & 63) + 18 > 64) w[(pos >> 6) + 1] += x >> (64 - (pos & 63));
    }
    Fr a; for (int i = 0; i < 8; i++) a.l[i] = (uint32_t)(w[i >> 1] >> (32 * (i & 1))); return a;
}

int main() {
    SIX_P = p_times(6); P13_10 = p_times(13, 10);
    // ---------------------------------------------------------------- 1. the full addition
    // (a) arbitrary field elements as coordinates (the formulas are polynomial identities), at and below the bounds of an accumulator
    for (int it = 0; it < 40000; it++) {
        XyzzW a, b;
        a.x = addn(rnd_w(), p_times(rnd() % 5)); a.y = addn(rnd_w(), p_times(rnd() % 5)); a.zz = rnd_w(); a.zzz = rnd_w();
        b.x = addn(rnd_w(), p_times(rnd() % 5)); b.y = addn(rnd_w(), p_times(rnd() % 5)); b.zz = rnd_w(); b.zzz = rnd_w();
        const int kind = it & 15;
        if (kind == 1) { a.x = minus_one(SIX_P); a.y = minus_one(SIX_P); a.zz = minus_one(P13_10); a.zzz = minus_one(P13_10); }
        if (kind == 2) { b.x = minus_one(SIX_P); b.y = minus_one(SIX_P); b.zz = minus_one(P13_10); b.zzz = minus_one(P13_10); }
        if (kind == 3) { a.x = b.x = minus_one(SIX_P); a.y = minus_one(SIX_P); a.zz = b.zz = minus_one(P13_10); b.zzz = minus_one(P13_10); }
        if (kind == 4) { a.x = limbs_at_max(SIX_P); a.y = limbs_at_max(SIX_P); a.zz = limbs_at_max(P13_10); a.zzz = limbs_at_max(P13_10); }         // every limb at its maximum
        if (kind == 5) { a.x = limbs_at_max(SIX_P); a.y = limbs_at_max(SIX_P); a.zz = limbs_at_max(P13_10); a.zzz = limbs_at_max(P13_10);
                         b.x = limbs_at_max(SIX_P); b.y = minus_one(SIX_P); b.zz = limbs_at_max(P13_10); b.zzz = minus_one(P13_10); }
        if (kind == 6) { a.x = w_zero<FqW>(); a.y = w_zero<FqW>(); }                           // (zz != 0: not the identity)
        if (kind == 7) { b.x = w_zero<FqW>(); b.y = w_zero<FqW>(); }
        if (kind == 8) a = xyzzw_identity();
        if (kind == 9) b = xyzzw_identity();
        if (kind == 10) { a = xyzzw_identity(); b = xyzzw_identity(); }
        both(a, b, "random coordinates");
    }
    // (b) curve points as the reduction meets them: bucket sums out of xyzzw_add_mixed_flag, sums of them, sums of sums, doublings
    G1Affine g; g.x = from_u64<FqParams>(1); g.y = from_u64<FqParams>(2);
    AffW ptsw[32];
    { G1Xyzz t = xyzz_from_affine(g); for (int i = 0; i < 32; i++) { ptsw[i] = aff_to_w(to_aff(t)); t = xyzz_double(t); xyzz_add_mixed(t, g, false); } }
    auto bucket = [&](int terms) {                             // a bucket's partial sum: `terms` mixed additions into a fresh accumulator
        XyzzW acc = xyzzw_identity(); bool fresh = true;
        for (int j = 0; j < terms; j++) xyzzw_add_mixed_flag(acc, fresh, ptsw[rnd() & 31], rnd() & 1);
        return acc;
    };
    XyzzW pool[16];
    for (int i = 0; i < 16; i++) pool[i] = bucket(1 + (int)(rnd() % 6));
    for (int it = 0; it < 70000; it++) {
        const int i = rnd() & 15, j = rnd() & 15, op = rnd() % 16;
        if (op < 7) pool[i] = both(pool[i], bucket((int)(rnd() % 5)), "sum + bucket");                                 // X += O  (O: a bucket, 0 terms = the identity)
        else if (op < 11) pool[i] = both(pool[i], pool[j], i == j ? "sum + itself" : "sum + sum");                     // Y += X, the tree steps; i == j: the doubling steps
        else if (op == 11) { XyzzW n = pool[j]; n.y = sub6(w_zero<FqW>(), n.y); const XyzzW z = both(pool[j], n, "P - P"); if (!is_inf(z) && !is_inf(pool[j])) { abad++; printf("P - P is not the identity\n"); } aid++; }
        else if (op == 12) {                                                                                             // the same point in other coordinates: P + P through the exact test
            if (is_inf(pool[j])) continue;
            G1Xyzz e; e.x = pack<FqParams>(s_from_w(pool[j].x)); e.y = pack<FqParams>(s_from_w(pool[j].y)); e.zz = pack<FqParams>(s_from_w(pool[j].zz)); e.zzz = pack<FqParams>(s_from_w(pool[j].zzz));
            const AffW q = aff_to_w(to_aff(e));
            XyzzW o; o.x = q.x; o.y = q.y; o.zz = w_one<FqW>(); o.zzz = w_one<FqW>();
            const XyzzW pj = pool[j];
            pool[i] = both(pj, o, "P + P (other coordinates)"); adbl++;
            o.y = neg2(o.y);
            const XyzzW z = both(pj, o, "P - P (other coordinates)");
            if (!is_inf(z)) { abad++; printf("P - P (other coordinates) is not the identity\n"); }
        }
        else if (op == 13) pool[i] = bucket(1 + (int)(rnd() % 6));
        else if (op == 14) pool[i] = both(xyzzw_identity(), pool[j], "identity + sum");
        else pool[i] = both(pool[j], xyzzw_identity(), "sum + identity");
    }
    // the walk has stayed on XYZZ coordinates: zz^3 == zzz^2
    for (int i = 0; i < 16; i++) if (!is_inf(pool[i])) { const FqW9 a = reduce_full(mulw(sqrw(pool[i].zz), pool[i].zz)), b = reduce_full(sqrw(pool[i].zzz)); if (!same(a, b)) { abad++; printf("zz^3 != zzz^2 at the end of the walk\n"); } }
    if (!limbs_ok) { abad++; printf("an operand exceeds its documented limb bound, or a folded difference is not the helper's\n"); }
    printf("full addition: %d mismatches in %d cases (%d on the hot path, %d doublings in other coordinates, %d P - P); largest column %.4f * 2^64\n",
           abad, acases, ahot, adbl, aid, (double)atop / 18446744073709551616.0);
    // ---------------------------------------------------------------- 2. scalars
    Fr r_minus_1; for (int i = 0; i < 8; i++) r_minus_1.l[i] = R_WORDS[i]; r_minus_1.l[0] -= 1;
    Fr one = fr_zero(); one.l[0] = 1;
    check_value(fr_zero(), "0"); check_value(one, "1"); check_value(r_minus_1, "r - 1");
    { Fr rr; for (int i = 0; i < 8; i++) rr.l[i] = R_WORDS[i]; check_input(rr, "r itself as input"); }
    for (int k = 0; k < 254; k++) { check_value(pow2(k), "2^k"); check_value(pow2m1(k), "2^k - 1"); }
    { Fr a = pow2m1(254); check_input(a, "2^254 - 1 as input"); for (int i = 0; i < 8; i++) a.l[i] = 0xffffffffu; check_input(a, "2^256 - 1 as input"); }
    const uint32_t top_r = 0x30644e72u >> 14;                  // r >> 238: the largest top window of a residue
    const uint32_t wv[] = {(1u << 16) - 1, 1u << 16, (1u << 16) + 1, (1u << 17) - 1, 1, 0};
    for (uint32_t v : wv) for (uint32_t top : {0u, 1u, (1u << 13) - 1, 1u << 13, top_r - 1, top_r}) check_value(windows(v, top), "window pattern");
    for (uint32_t top = 1; top <= top_r; top += (top < 64 || top + 64 > top_r) ? 1 : 97) check_value(windows(0, top), "top window only");
    // (the carry into the top window: windows 0..13 all at 2^16 carry one into it)
    for (int it = 0; it < 120000; it++) {
        Fr a; for (int i = 0; i < 8; i++) a.l[i] = rnd();
        if (it & 1) { a.l[7] &= 0x3fffffffu; if (!below_r(a)) a.l[7] &= 0x1fffffffu; check_value(a, "random residue"); }
        else check_input(a, "random 256-bit word");
    }
    printf("scalars: %d mismatches in %d cases\n", sbad, scases);
    return (abad + sbad) ? 1 : 0;
}
