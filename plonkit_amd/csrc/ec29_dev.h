// G1 arithmetic over the 9 x 29-bit lazy field layer (field29_dev.h) — the MSM's inner loops.
// Same formulas as ec_dev.h (XYZZ coordinates: madd-2008-s, add-2008-s, dbl-2008-s-1), but every
// subtraction is a limb-wise "a - b + k*p" and nothing is conditionally reduced.  Invariants
// (values as multiples of p; all limbs normalised):
//     affine input       x, y      < 1.1 p     (resident SRS: canonical, 2^261 domain)
//     XYZZ accumulator   x, y      < 6 p       zz, zzz < 1.3 p
// Bound bookkeeping (out of mulw < a*b*0.0059/p + p):
//   madd:  U2,S2 < 1.02  P = U2-X+6p < 7.02  R = 8p-Y(+/-)S2 < 9.1  PP < 1.3  PPP < 1.06  Q < 1.05
//          X3 = R^2-PPP-2Q+4p < 5.5   T = Q-X3+6p < 7.05   Y3 = R*T + Y*(2p-PPP) (one reduction) < 1.5
//   add :  U,S < 1.05  P,R < 3.05  PP < 1.06  X3 < 5.06  Y3 < 3.2
//   dbl :  U = 2Y < 12  V < 1.85  W < 1.14  S < 1.07  M = 3X^2 < 3.7  X3 < 5.1  Y3 < 3.2
// The two additions priced by instruction count (xyzzw_add_mixed_flag, xyzzw_add_pairs) take their products with lazy Montgomery digits
// (field29_dev.h: *_lz): every product there is below the figure above + 2^-26 p, which no bound above notices (the tightest slack is
// R < 9.1 of 16 for maybe_zero_mod_p); the integers are the masked forms' or, about once in 2^26 products, larger by exactly p.
#pragma once
#include "field29_dev.h"
#include "ec_dev.h"

namespace plk {

struct AffW { FqW9 x, y; };
struct alignas(16) XyzzW { FqW9 x, y, zz, zzz; };              // 144 bytes

// the product is inlined: 162 v_mad_u64_u32 + ~60 other instructions (1.9 KB), ten of them per
// mixed addition keep the accumulate loop at ~25 KB, inside the 64 KB instruction cache
#define WM(a, b) mulw<FqW>((a), (b))
#define WS(a) sqrw<FqW>((a))                               // normalised input; 126 mads instead of 162
#define WMA(a, b, c, d) mul2addw<FqW>((a), (b), (c), (d))  // a*b + c*d, one reduction
// the latency-bound chains (full addition, doubling: bucket reduction, table build) take the operand-scanning forms
#define WMA_LZ(a, b, c, d) mul2addw_lz<FqW, LZ_ALL, LbNorm, LbT, LbNorm, LbNppp>((a), (b), (c), (d))   // the fused Y3 of the work-priced additions
#define WMA_LZF(a, b, c, d, FD) mul2addw_lz<FqW, LZ_ALL, LbNorm, LbT, LbNorm, LbNppp, (FD)>((a), (b), (c), (d))   // the same with the digits of FD folded
#define LM(a, b) mulw_os<FqW>((a), (b))
#define LS(a) sqrw_os<FqW>((a))
#define LMA(a, b, c, d) mul2addw_os<FqW>((a), (b), (c), (d))

// Declared limb bounds of the operands that the lazy-digit products (field29_dev.h: *_lz) of xyzzw_add_mixed_flag and xyzzw_add_pairs take
// un-normalised; every other operand there is LbNorm.  Each instantiation checks its exact per-column worst case at these bounds at compile time.
struct LbSignedY { static constexpr Limbs9 B = lb_max(LbNorm::B, lb_of(FqW::PAD2)); };     // +-y: y, or 2p - y as it stands (limbs <= PAD2's)
struct LbT { static constexpr Limbs9 B = lb_plus(lb_of(FqW::PAD6N), M29); };               // T = Q + (6p - X3) from PAD6N; Q, X3 normalised
struct LbNppp { static constexpr Limbs9 B = lb_of(FqW::PAD2N); };                          // 2p - PPP from PAD2N; PPP normalised

PLK_HD bool is_inf(const XyzzW &p) { return w_all_zero(p.zz); }
PLK_HD bool is_inf(const AffW &p) { return w_all_zero(p.x) && w_all_zero(p.y); }
PLK_HD XyzzW xyzzw_identity() { XyzzW r; r.x = w_zero<FqW>(); r.y = w_zero<FqW>(); r.zz = w_zero<FqW>(); r.zzz = w_zero<FqW>(); return r; }

// 2 * (x, y) for an affine point; ysgn selects +y / -y
PLK_HD XyzzW xyzzw_double_affine(const FqW9 &x, const FqW9 &y) {
    FqW9 u = addn(y, y), v = WS(u), w = WM(u, v), s = WM(x, v);
    FqW9 xx = WS(x), m = normw(addw(addw(xx, xx), xx));
    XyzzW r;
    r.x = sub4(WS(m), addn(s, s));
    r.y = WMA(m, sub6(s, r.x), y, neg2(w));
    r.zz = v; r.zzz = w;
    return r;
}

PLK_HD XyzzW xyzzw_double(const XyzzW &p) {
    if (is_inf(p)) return p;
    FqW9 u = addn(p.y, p.y), v = LS(u), w = LM(u, v), s = LM(p.x, v);
    FqW9 xx = LS(p.x), m = normw(addw(addw(xx, xx), xx));
    XyzzW r;
    r.x = sub4(LS(m), addn(s, s));
    r.y = LMA(m, sub6(s, r.x), p.y, neg2(w));
    r.zz = LM(v, p.zz); r.zzz = LM(w, p.zzz);
    return r;
}

// slow path of the mixed addition: the x-difference passed the cheap zero filter.  Recomputes the
// exact tests; falls back to the generic addition when the filter was a false positive.
PLK_HD void xyzzw_add(XyzzW &a, const XyzzW &b);
// (inlined on purpose: a non-inlined callee is compiled with its own 200+ VGPR budget, which the
//  AMDGPU backend then charges to every kernel that can reach it — halving the occupancy of the hot loop)
PLK_HD void xyzzw_add_mixed_special(XyzzW &acc, const AffW &q, bool neg_q, const FqW9 &p, const FqW9 &r) {
    if (is_zero_mod_p(p)) {
        if (is_zero_mod_p(r)) acc = xyzzw_double_affine(q.x, neg_q ? neg2(q.y) : q.y);
        else acc = xyzzw_identity();
        return;
    }
    XyzzW t; t.x = q.x; t.y = neg_q ? neg2(q.y) : q.y; t.zz = w_one<FqW>(); t.zzz = w_one<FqW>();
    xyzzw_add(acc, t);
}

// acc += (qx, +-qy)
PLK_HD void xyzzw_add_mixed(XyzzW &acc, const AffW &q, bool neg_q) {
    if (is_inf(q)) return;
    if (is_inf(acc)) { acc.x = q.x; acc.y = neg_q ? neg2(q.y) : q.y; acc.zz = w_one<FqW>(); acc.zzz = w_one<FqW>(); return; }
    FqW9 u2, s2;
    mulw2<FqW>(q.x, acc.zz, q.y, acc.zzz, u2, s2);
    FqW9 p = sub6(u2, acc.x);
    FqW9 r;
    {
        const uint32_t m = neg_q ? 0xffffffffu : 0u;
#pragma unroll
        for (int i = 0; i < 9; i++) r.l[i] = FqW::PAD8[i] - acc.y.l[i] + ((s2.l[i] ^ m) - m);
        r = normw(r);
    }
    if (maybe_zero_mod_p(p)) {                               // P == +-Q: rare, kept out of the hot code
        xyzzw_add_mixed_special(acc, q, neg_q, p, r);
        return;
    }
    FqW9 pp, rr, ppp, qq;
    sqrw2<FqW>(p, r, pp, rr);
    mulw2<FqW>(p, pp, acc.x, pp, ppp, qq);
    FqW9 x3;
    {
#pragma unroll
        for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
        x3 = normw(x3);
    }
    FqW9 zz3, zzz3;
    mulw2<FqW>(acc.zz, pp, acc.zzz, ppp, zz3, zzz3);
    acc.y = WMA(r, sub6(qq, x3), acc.y, neg2(ppp));           // R*(Q - X3) - Y*PPP, one reduction
    acc.x = x3;
    acc.zz = zz3;
    acc.zzz = zzz3;
}

// The same addition for the flat loop of msm_accumulate's plain kernel, with less work around the ten products.  The same point mod p in
// every coordinate (tests/host/field29_addend_check.hip holds the earlier form, tests/host/field29_lazy_digits_check.hip the one with masked digits).
//   - No is_inf(q): the caller runs this only over a table that holds no point at infinity (msm.hip establishes that where it builds the
//     table).  is_inf(acc), an OR over nine limbs in every addition, is the lane flag `fresh`: the caller sets it where it sets acc to
//     the identity (start, after a flush); it is cleared by the first point taken and set again where the special path returns the
//     identity.  (A hot-path result is never the identity: zz3 = 0 needs P = 0 mod p, and maybe_zero_mod_p has no false negatives.)
//   - P = U2 + (6p - X) and R = S2 + (8p - Y) come out of the product pair itself (mulw2_add): the padded terms are addends of the high
//     columns, whose carry chain normalises the sums, so neither sub6 nor normw follows.  Values as before: P < 7.02, R < 9.1.
//   - The sign of y goes onto the affine operand BEFORE the product: +-y is y or the raw 2p - y (limbs <= PAD2's 2.63e9, below
//     MULW_A_LIMB_MAX; value < 2p, so S2 < 2 * 1.3 * 0.0059 + 1 < 1.02 as before).  For a negated y this R differs from the earlier
//     8p - Y - y*zzz by a multiple of p.
//   - T = Q - X3 + 6p and 2p - PPP enter the fused Y3 product as they stand, without normw: they are its RIGHT operands, taken from the
//     pads with the 2^29 bias (PAD6N, PAD2N: X3 and PPP are normalised), so their limbs stay below 1.45e9 and 1.02e9; R and Y are
//     normalised, and a column holds at most 9 * (2^29 * 1.45e9 + 2^29 * 1.02e9 + (2^29)^2) + 2^35 < 0.79 * 2^64 (host-checked with a
//     128-bit shadow of the chain at exactly these limbs).  With the 2^31 pads the same column reaches 1.6 * 2^64.
//   - Lazy Montgomery digits in all nine reductions (mulw2_add_lz, sqrw2_lz, mulw2_lz twice, mul2addw_lz; LZ_ALL: m_0..m_7 unmasked, 72
//     v_and_b32 fewer per addition).  Every operand is normalised (LbNorm) except +-y (LbSignedY: limbs <= PAD2's), the two addends (LbAny) and
//     the right operands T and 2p - PPP of the fused Y3 (LbT, LbNppp: the 2^29-bias pads).  Exact worst columns at those bounds, checked at
//     compile time: 0.50 * 2^64 for the normalised products and squarings, 0.92 * 2^64 for the +-y chain with its addend, 0.85 * 2^64 for Y3.
//     (A uniform bound over the left operand, 9 * 2.63e9 * 2^29, would put the +-y chain at 2^64.09; limb by limb PAD2 sums to 18.8e9, not 23.7e9.)
// Not folded: X3 = R^2 + (4p - PPP - 2Q) needs R^2 after PPP and Q; the lockstep pairs would have to become PP alone, (PPP, Q),
// (R^2 + addend, ZZ*PP), ZZZ*PPP alone — two single chains, whose wait states only the second wave hides, for ~25 instructions.
// NXY (the loop of msm_accumulate's plain kernel): acc.x and acc.y hold NX = -X and NY = -Y (mod p) between the additions, zz and zzz as
// they are.  The padded 6p - X and 8p - Y that P and R take as addends are then the coordinates themselves and are not formed (18
// subtractions an iteration): P = U2 + NX, R = S2 + NY.  NQ = NX * PP = -Q, so NX3 = PPP + 2Q - R^2 = PPP - 2 NQ - R^2 + 4p, and
// NY3 = -(R (Q - X3) - Y PPP) = R (NQ - NX3 + 6p) + NY (2p - PPP): the same fused product with the same pads.  Bounds: R^2 < 1.5p and
// 2 NQ < 2.1p leave NX3 positive and below 5.06p, so P < 6.1p; NY3 < 1.5p, a first point enters as 2p - x and 2p -+ y (< 2p): R < 3.1p.
// xyzzw_flip_xy converts in both directions (6p - c: an accumulator's x, y < 6p on either side) where the sum leaves the loop (the flush)
// and around the cold P = +-Q path.  The identity is zz = 0 whatever x and y hold: the one that path returns carries 6p - 0 in both
// and flips back to all zero (keeping it zero in place costs the hot path 24 moves: two values merge at the loop's head).
// SF (the loop of msm_accumulate's plain kernel, together with NXY): the SHARED FACTOR PP = P^2 is the right operand of three products - PPP = P PP,
// Q = X1 PP (here NQ = NX PP), ZZ3 = ZZ1 PP - and is reduced once for the three: A_PP = PP 2^-116 mod p (make_tw2_a, 39 multiply-adds), then each is a
// tw2 product (field29_dev.h: 126 multiply-adds instead of 162), (PPP, NQ) as a lockstep pair and ZZ3 beside the plain product ZZZ3 = ZZZ1 PPP
// (mul_tw2_mulw).  1483 -> 1414 multiply-adds an addition.  The same residues in all four coordinates, not the same integers.  Operands: P, NX, ZZ1 and
// PP are normalised (out of a column chain or normw), A_PP is LbTw2A; worst column 0.43 * 2^64, checked at compile time.  Values: a tw2 result is below
// z w / 2^261 + A / 2^29 + p (1 + 2^-26), i.e. the bound of the mulw2_lz it replaces + 2^-28 p: PPP < 1.06, Q < 1.05, ZZ3 < 1.01 as in the table above
// (tests/host/field29_shared_factor_check.hip: chains of 250 additions from accumulators at the coordinate bounds, this form beside <true, false>).
// FOLDED DIGITS (with SF, i.e. in <true, true> only; field29_dev.h, "THE FOLD"): the low digits of all ten reductions are divided out by FqW::FOLDC = 2^-29 mod p
// + 2p instead of a Montgomery step - digits 0..6 of the six nine-digit reductions (FOLD9: the pair (P, R), the squaring pair, ZZZ3 beside ZZ3, the fused Y3),
// 0..2 of the three tw2 chains (FOLD_TW2), 0..1 of A_PP (FOLD_TW2A): 53 of the 74 v_mul_lo_u32 of an addition are not issued, and the column shift of a
// folded digit is a multiply-add of the accumulator's high word by eight.  Values: a folded reduction's result is below the unfolded form's bound
// + 2^32 FOLDC / 2^58 (1 + 2^-28) < + 2.15 * 2^-26 p, so every product here is below its figure in the table at the top + 3.2 * 2^-26 p (lazy and folded
// together): U2, S2 < 1.02, PP < 1.3, PPP < 1.06, Q < 1.05, ZZ3, ZZZ3 < 1.01, NY3 < 1.5, P < 6.1 and R < 9.1 of maybe_zero_mod_p's 16 - no bound above notices.
// The integers are the unfolded form's unless a result crosses a multiple of p in that margin (then they differ by p; about once in 2^25 products).
// Columns, exact worst cases at the declared bounds (checked at compile time): 0.426 * 2^64 for the normalised products and squarings (0.501 unfolded),
// 0.848 for the +-y chain with its addend (0.923), 0.771 for Y3 (0.845), 0.372 for tw2 (0.425), 0.181 for A_PP (0.211): FOLDC's limbs are smaller than p's.
// tests/host/field29_fold_check.hip: every folded form against mulw, and chains of 250 additions of this form beside the unfolded one.
PLK_HD XyzzW xyzzw_flip_xy(const XyzzW &a) { XyzzW r = a; r.x = sub6(w_zero<FqW>(), a.x); r.y = sub6(w_zero<FqW>(), a.y); return r; }
template <bool NXY, bool SF = false>
PLK_HD void xyzzw_add_mixed_flag_impl(XyzzW &acc, bool &fresh, const AffW &q, bool neg_q) {
    if (fresh) {
        if constexpr (NXY) { acc.x = neg2(q.x); acc.y = neg_q ? q.y : neg2(q.y); }
        else { acc.x = q.x; acc.y = neg_q ? neg2(q.y) : q.y; }
        acc.zz = w_one<FqW>(); acc.zzz = w_one<FqW>(); fresh = false; return;
    }
    constexpr unsigned F9 = SF ? FOLD9 : 0u, F5 = SF ? FOLD_TW2 : 0u, F4 = SF ? FOLD_TW2A : 0u;   // the fold sets of the nine-, five- and four-digit reductions
    FqW9 p, r, yq;
#pragma unroll
    for (int i = 0; i < 9; i++) yq.l[i] = neg_q ? FqW::PAD2[i] - q.y.l[i] : q.y.l[i];           // 2p - y (limbs <= 2.63e9 < MULW_A_LIMB_MAX, value < 2p) or y
    if constexpr (NXY) mulw2_add_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbSignedY, LbNorm, LbNorm, F9>(q.x, acc.zz, acc.x, yq, acc.zzz, acc.y, p, r);   // P = U2 + NX,  R = S2 + NY
    else {
        FqW9 ax, ay;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            ax.l[i] = FqW::PAD6[i] - acc.x.l[i];                         // 6p - X, 8p - Y: limbs <= the pads' (< 2^32), not normalised
            ay.l[i] = FqW::PAD8[i] - acc.y.l[i];
        }
        mulw2_add_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbAny, LbSignedY, LbNorm, LbAny>(q.x, acc.zz, ax, yq, acc.zzz, ay, p, r);          // P = U2 + (6p - X),  R = S2 + (8p - Y)
    }
    if (maybe_zero_mod_p(p)) {                               // P == +-Q: rare, kept out of the hot code
        AffW t; t.x = q.x; t.y = normw(yq);                    // (+-y as xyzzw_add_mixed forms it: neg2(y) = normw(2p - y), y is normalised)
        if constexpr (NXY) acc = xyzzw_flip_xy(acc);
        xyzzw_add_mixed_special(acc, t, false, p, r);
        fresh = is_inf(acc);
        if constexpr (NXY) acc = xyzzw_flip_xy(acc);
        return;
    }
    FqW9 pp, rr, ppp, qq;
    sqrw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, F9>(p, r, pp, rr);
    FqW9 a_pp;
    if constexpr (SF) {
        a_pp = make_tw2_a<FqW, TW2A_LZ_ALL, LbNorm, F4>(pp);
        mul_tw2_2<FqW, TW2_LZ_ALL, TW2_LZ_ALL, LbNorm, LbNorm, LbTw2A, LbNorm, F5>(p, a_pp, pp, acc.x, a_pp, pp, ppp, qq);
    } else
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm>(p, pp, acc.x, pp, ppp, qq);            // (NXY: qq = NQ = -Q)
    FqW9 x3;
    {
#pragma unroll
        for (int i = 0; i < 9; i++) x3.l[i] = NXY ? ppp.l[i] + FqW::PAD4[i] - rr.l[i] - 2 * qq.l[i] : rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
        x3 = normw(x3);
    }
    FqW9 zz3, zzz3;
    if constexpr (SF) {
        mul_tw2_mulw<FqW, TW2_LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbTw2A, LbNorm, F5, F9>(acc.zz, a_pp, pp, acc.zzz, ppp, zz3, zzz3);
    } else
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm>(acc.zz, pp, acc.zzz, ppp, zz3, zzz3);
    FqW9 t, nppp;
#pragma unroll
    for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; nppp.l[i] = FqW::PAD2N[i] - ppp.l[i]; }
    acc.y = WMA_LZF(r, t, acc.y, nppp, F9);                   // R*(Q - X3) - Y*PPP, one reduction (NXY: R*(NQ - NX3) - NY*PPP = NY3)
    acc.x = x3;
    acc.zz = zz3;
    acc.zzz = zzz3;
}
PLK_HD void xyzzw_add_mixed_flag(XyzzW &acc, bool &fresh, const AffW &q, bool neg_q) { xyzzw_add_mixed_flag_impl<false>(acc, fresh, q, neg_q); }
PLK_HD void xyzzw_add_mixed_nflag(XyzzW &acc, bool &fresh, const AffW &q, bool neg_q) { xyzzw_add_mixed_flag_impl<true, true>(acc, fresh, q, neg_q); }

// a += b
PLK_HD void xyzzw_add(XyzzW &a, const XyzzW &b) {
    if (is_inf(b)) return;
    if (is_inf(a)) { a = b; return; }
    FqW9 u1 = LM(a.x, b.zz), u2 = LM(b.x, a.zz), s1 = LM(a.y, b.zzz), s2 = LM(b.y, a.zzz);
    FqW9 p = sub2(u2, u1), r = sub2(s2, s1);
    if (is_zero_mod_p(p)) {
        if (is_zero_mod_p(r)) a = xyzzw_double(a);
        else a = xyzzw_identity();
        return;
    }
    FqW9 pp = LS(p), ppp = LM(p, pp), qq = LM(u1, pp);
    FqW9 x3;
    {
        FqW9 rr = LS(r);
#pragma unroll
        for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
        x3 = normw(x3);
    }
    a.y = LMA(r, sub6(qq, x3), s1, neg2(ppp));
    a.x = x3;
    a.zz = LM(LM(a.zz, b.zz), pp);
    a.zzz = LM(LM(a.zzz, b.zzz), ppp);
}

// a += b for the WORK-bound bucket reduction (msm_task_reduce<.., PAIRS>: a batch of three or more, or other commitments in flight — two of
// these chains per SIMD beside another commitment's accumulation, priced by the instructions they issue, not by their latency): the same
// fourteen products as xyzzw_add, issued as the lockstep product-scanning pairs of the mixed addition (~205 instructions per product against
// ~243 of a lone operand-scanning chain) and the fused Y3 as one product-scanning chain.  The same residues as xyzzw_add in all four
// coordinates, and the same integers unless a lazy multiplier passes 2^261 (then larger by p): mulw / sqrw / mul2addw and their _os forms
// return the same normalised (a*b + m*p) / 2^261, and the two folds below keep the integers (tests/host/field29_pairs_check.hip: > 10^5
// operands as the reduction feeds them in, every chain shadowed in 128 bits; tests/host/field29_lazy_digits_check.hip for the lazy digits).
//   - Pairs: (U1, S1), (U2, S2), (ZZ1*ZZ2, ZZZ1*ZZZ2), (PP, RR) as squarings, (PPP, Q), (ZZ3, ZZZ3).  U1 and S1 go first because
//   - P = U2 + (2p - U1) and R = S2 + (2p - S1) come out of the second pair itself (mulw2_add): the padded differences are addends of its
//     high columns, whose carry chain normalises the sums — bit for bit sub2(U2, U1) and sub2(S2, S1), without their 9 additions and normw.
//     Addend limbs <= PAD2's (< 2^32; >= 0: U1, S1 are normalised and below 2p), less than 16p added to a product below 1.1p, as mulw2_add asks.
//   - T = Q - X3 + 6p and 2p - PPP enter the fused Y3 product as they stand, from the pads with the 2^29 bias, as in xyzzw_add_mixed_flag:
//     right operands with limbs below 1.45e9 and 1.02e9 (X3, PPP, Q normalised) beside the normalised left operands R and S1: the column
//     bound derived there, < 0.79 * 2^64.  mul2addw sees the same integers as with sub6 / neg2, so the result is the same.
// Bounds.  Every other operand of every product here is NORMALISED (limbs < 2^29; the top limb too, the values being far below 2^261): the
// coordinates come out of a product's column chain or of normw (outputs of xyzzw_add_mixed_flag, of this addition or of xyzzw_double: x,
// y < 6p, zz, zzz < 1.3p), P and R out of the column chain of mulw2_add (P, R < 3.05p).
//   - mulw2 / mulw2_add, left operands X1, Y1, X2, Y2, ZZ1, ZZZ1, P, U1, ZZ1*ZZ2, ZZZ1*ZZZ2: limbs < 2^29, far below MULW_A_LIMB_MAX = 3.28e9;
//     a column holds at most 2 * 9 * (2^29 - 1)^2 + 2^35 (+ 2^32 for an addend) < 2^62.2.
//   - sqrw2 of (P, R): the doubled limbs stay below 2^30, a column at most 9 * (2^30 * 2^29 + 2^58) + 2^35 < 2^62.8.
//   - Lazy Montgomery digits in all thirteen reductions (LZ_ALL, 104 v_and_b32 fewer): the normalised operands above are LbNorm, the addends
//     LbAny, T and 2p - PPP LbT and LbNppp; worst columns as in xyzzw_add_mixed_flag (0.50 * 2^64 normalised, 0.85 * 2^64 for Y3), checked at
//     compile time.  Values grow by less than 2^-26 p per product: is_zero_mod_p's a < 16p holds with P, R < 3.05p as before.
//   - Folded digits (field29_dev.h, "THE FOLD"): digits 0..6 of all thirteen reductions (FOLD9) are divided out by FqW::FOLDC instead of a Montgomery step, 91
//     v_mul_lo_u32 fewer; each result is below the lazy form's bound + 2.15 * 2^-26 p, and its integer is the lazy form's unless it crosses a multiple of p in
//     that margin - tests/host/field29_pairs_check.hip still finds xyzzw_add's integers in all of its 10^5 cases.  Worst columns 0.426 * 2^64 (normalised
//     products, squarings, the pair with its LbAny addends) and 0.771 (Y3), checked at compile time; tests/host/field29_fold_check.hip holds chains of 250 of
//     these additions beside the unfolded form.
// Values: U, S < 6 * 1.3 * 0.0059p + p < 1.05p; PP < 3.05^2 * 0.0059p + p < 1.06p; X3 < 5.06p; Y3 < (3.05 * 7.1 + 1.05 * 2) * 0.0059p + p < 1.2p (each + 3.2 * 2^-26 p).
PLK_HD void xyzzw_add_pairs(XyzzW &a, const XyzzW &b) {
    if (is_inf(b)) return;
    if (is_inf(a)) { a = b; return; }
    FqW9 u1, s1, p, r;
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm, FOLD9>(a.x, b.zz, a.y, b.zzz, u1, s1);
    {
        FqW9 nu, ns;
#pragma unroll
        for (int i = 0; i < 9; i++) { nu.l[i] = FqW::PAD2[i] - u1.l[i]; ns.l[i] = FqW::PAD2[i] - s1.l[i]; }     // 2p - U1, 2p - S1: not normalised
        mulw2_add_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbAny, LbNorm, LbNorm, LbAny, FOLD9>(b.x, a.zz, nu, b.y, a.zzz, ns, p, r);
    }
    if (is_zero_mod_p(p)) {
        if (is_zero_mod_p(r)) a = xyzzw_double(a);
        else a = xyzzw_identity();
        return;
    }
    FqW9 zz12, zzz12;
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm, FOLD9>(a.zz, b.zz, a.zzz, b.zzz, zz12, zzz12);
    FqW9 pp, rr, ppp, qq;
    // (P and R are hidden from the optimiser here: knowing from the chain's masks that their limbs are below 2^29, it widens the squarings'
    //  doubled limbs "x << 1" to 33-bit values and pays two multiply-adds and two moves for each of ~100 products)
#pragma unroll
    for (int i = 0; i < 9; i++) { PLK_CHAIN(p.l[i]); PLK_CHAIN(r.l[i]); }
    sqrw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, FOLD9>(p, r, pp, rr);
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm, FOLD9>(p, pp, u1, pp, ppp, qq);
    FqW9 x3;
    {
#pragma unroll
        for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
        x3 = normw(x3);
    }
    FqW9 t, nppp;
#pragma unroll
    for (int i = 0; i < 9; i++) { t.l[i] = qq.l[i] + FqW::PAD6N[i] - x3.l[i]; nppp.l[i] = FqW::PAD2N[i] - ppp.l[i]; }
    a.y = WMA_LZF(r, t, s1, nppp, FOLD9);                     // R*(Q - X3) - S1*PPP, one reduction
    a.x = x3;
    mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbNorm, LbNorm, LbNorm, LbNorm, FOLD9>(zz12, pp, zzz12, ppp, a.zz, a.zzz);
}

// storage <-> registers
__device__ __forceinline__ AffW load_affw(const G1Affine *p) {            // packed, already in the 2^261 domain
    AffW r; r.x = unpack<FqW>(load_fp(&p->x)); r.y = unpack<FqW>(load_fp(&p->y)); return r;
}
__device__ __forceinline__ FqW9 load_w(const uint32_t *p) {
    FqW9 r;
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    u32x4 a = q[0], b = q[1];
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w; r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w; r.l[8] = p[8];
    return r;
}
__device__ __forceinline__ void store_w(uint32_t *p, const FqW9 &v) {
    u32x4 *q = reinterpret_cast<u32x4 *>(p);
    q[0] = u32x4{v.l[0], v.l[1], v.l[2], v.l[3]};
    q[1] = u32x4{v.l[4], v.l[5], v.l[6], v.l[7]};
    p[8] = v.l[8];
}
// XyzzW in memory: 4 coordinates x (8 limbs in two 16-byte words + the 9th in a trailing block) = 144 B
__device__ __forceinline__ XyzzW load_xyzzw(const XyzzW *p) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    XyzzW r;
    FqW9 *c[4] = {&r.x, &r.y, &r.zz, &r.zzz};
    u32x4 tail = *reinterpret_cast<const u32x4 *>(w + 32);
    const uint32_t t[4] = {tail.x, tail.y, tail.z, tail.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32x4 *q = reinterpret_cast<const u32x4 *>(w + 8 * k);
        u32x4 a = q[0], b = q[1];
        c[k]->l[0] = a.x; c[k]->l[1] = a.y; c[k]->l[2] = a.z; c[k]->l[3] = a.w;
        c[k]->l[4] = b.x; c[k]->l[5] = b.y; c[k]->l[6] = b.z; c[k]->l[7] = b.w; c[k]->l[8] = t[k];
    }
    return r;
}
__device__ __forceinline__ void store_xyzzw(XyzzW *p, const XyzzW &v) {
    uint32_t *w = reinterpret_cast<uint32_t *>(p);
    const FqW9 *c[4] = {&v.x, &v.y, &v.zz, &v.zzz};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u32x4 *q = reinterpret_cast<u32x4 *>(w + 8 * k);
        q[0] = u32x4{c[k]->l[0], c[k]->l[1], c[k]->l[2], c[k]->l[3]};
        q[1] = u32x4{c[k]->l[4], c[k]->l[5], c[k]->l[6], c[k]->l[7]};
    }
    *reinterpret_cast<u32x4 *>(w + 32) = u32x4{v.x.l[8], v.y.l[8], v.zz.l[8], v.zzz.l[8]};
}

// XYZZ (2^261 domain, lazy) -> XYZZ in the library's external form (canonical, R = 2^256), for the host
__device__ __forceinline__ G1Xyzz xyzzw_export(const XyzzW &p) {
    G1Xyzz r;
    if (is_inf(p)) return xyzz_identity();
    r.x = pack<FqParams>(s_from_w(p.x)); r.y = pack<FqParams>(s_from_w(p.y));
    r.zz = pack<FqParams>(s_from_w(p.zz)); r.zzz = pack<FqParams>(s_from_w(p.zzz));
    return r;
}

}  // namespace plk
