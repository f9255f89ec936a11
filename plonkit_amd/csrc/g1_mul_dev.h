// Scalar multiplication of a G1 point on the 9 x 29-bit lazy layer — the butterflies of the inverse NTT over G1 (g1ntt.hip); a header of
// its own so that the known-answer driver (tests/host/arith_kat.hip) can call the three variants and their mixed addition directly.
// Every function here takes its window table in LDS, limb-major: `tab` is the workgroup's dynamic shared memory, G1NTT_THREADS lanes wide,
// G1NTT_LDS / G1NTT_LDS_ISO / G1NTT_LDS_ISO8 bytes for g1_mul_scalar / g1_mul_scalar_iso / g1_mul_scalar_iso8.
#pragma once
#include "ec_dev.h"
#include "ec29_dev.h"
#include "glv_dev.h"

namespace plk {

constexpr int G1NTT_THREADS = 256;
constexpr int G1NTT_TABLE = 4;                                     // |digit| <= 4
constexpr size_t G1NTT_LDS = (size_t)G1NTT_TABLE * 36 * G1NTT_THREADS * sizeof(uint32_t);   // 147456 B: one workgroup per CU

// rarely executed additions / doublings go through one out-of-line copy each (code size); the loop has its own inlined sites
__device__ __noinline__ void g1_add_call(XyzzW *a, const XyzzW *b) { XyzzW t = *a; xyzzw_add(t, *b); *a = t; }
__device__ __noinline__ void g1_double_call(XyzzW *a) { XyzzW t = *a; *a = xyzzw_double(t); }

__device__ __forceinline__ void lds_put(uint32_t *tab, int e, const XyzzW &p) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(&p);
#pragma unroll
    for (int k = 0; k < 36; k++) tab[(e * 36 + k) * G1NTT_THREADS + threadIdx.x] = w[k];
}
__device__ __forceinline__ XyzzW lds_get(const uint32_t *tab, int e) {
    XyzzW p;
    uint32_t *w = reinterpret_cast<uint32_t *>(&p);
#pragma unroll
    for (int k = 0; k < 36; k++) w[k] = tab[(e * 36 + k) * G1NTT_THREADS + threadIdx.x];
    return p;
}

// k * b for a canonical (non-Montgomery) scalar k < r, by the GLV endomorphism (glv_dev.h): k = k1 + k2 lambda with
// |k1|, |k2| < 2^128 and lambda * (x, y) = (beta x, y), so both halves share ONE chain of 129 doublings:
//     acc <- 8 acc ; acc += d1_w * b ; acc += d2_w * phi(b)          for the 43 signed 3-bit windows, high to low,
// d in [-3, 4] as in round 1, phi of a table entry = its x times beta (one more product).  129 doublings + 86 additions + 43
// products by beta = ~2400 field products per multiplication instead of the ~3500 of 255 doublings + 85 additions.  The two
// additions of a window go through ONE inlined addition site (a two-trip loop that is not unrolled: instruction cache).
__device__ __forceinline__ XyzzW g1_mul_scalar(const XyzzW &b, const Fr &k, uint32_t *tab) {
    if (is_inf(b)) return xyzzw_identity();
    {   // table: b, 2b, 3b, 4b
        XyzzW t = b, t2 = b;
        lds_put(tab, 0, t);
        g1_double_call(&t2);
        lds_put(tab, 1, t2);
        t = t2; g1_add_call(&t, &b);
        lds_put(tab, 2, t);
        g1_double_call(&t2);
        lds_put(tab, 3, t2);
    }
    uint32_t dig[2][6];
    uint32_t flip[2];                                             // sign of the half: XORed into the digit's sign bit
    {
        const GlvSplit sp = glv_split(k.l);
        glv_digits(sp.k1, dig[0]);
        glv_digits(sp.k2, dig[1]);
        flip[0] = sp.neg1 ? 8u : 0u; flip[1] = sp.neg2 ? 8u : 0u;
    }
    FqW9 beta;
#pragma unroll
    for (int i = 0; i < 9; i++) beta.l[i] = glv::BETA_W[i];
    XyzzW acc = xyzzw_identity();
    for (int w = 42; w >= 0; w--) {
        for (int r = 0; r < 3; r++) acc = xyzzw_double(acc);      // one inlined doubling site (identity passes through)
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            const uint32_t code = ((dig[h][w >> 3] >> (4 * (w & 7))) & 15u), mag = code & 7u;
            XyzzW t = xyzzw_identity();
            if (mag) {
                t = lds_get(tab, (int)mag - 1);
                if (h) t.x = WM(t.x, beta);                        // phi: x -> beta x (entries are normalised, x < 6p -> < 1.04p)
                if ((code ^ flip[h]) & 8u) t.y = sub6(w_zero<FqW>(), t.y);     // 6p - y: y < 6p by the bounds of ec29_dev.h
            }
            xyzzw_add(acc, t);                                    // the one inlined addition site (identity operand: no-op)
        }
    }
    return acc;
}

// ---- the same multiplication with an EFFECTIVELY AFFINE window table (late round 6).  The four table points b, 2b, 3b, 4b are brought to ONE
// denominator pair (D_zz = prod ZZ_i, D_zzz = prod ZZZ_i: x_i = X_i' / D_zz, y_i = Y_i' / D_zzz with X_i' = X_i prod_{j != i} ZZ_j, 22 products), and the whole
// double-and-add runs on the isomorphic curve (x, y) -> (x D_zz, y D_zzz) — for a = 0 neither the addition nor the doubling formulas contain a curve constant —
// where the table points are AFFINE: 86 MIXED additions of 10 products instead of 86 full additions of 14, table entries of 18 words instead of 36 in LDS,
// and two products at the end take the accumulator back (ZZ D_zz, ZZZ D_zzz).  129 doublings + 86 mixed additions + 43 products by beta + 56 for the table
// = ~2100 field products instead of ~2400.  The mixed addition is ec29_dev.h's in the operand-scanning forms (a lone wave per SIMD: field29_dev.h).
PLK_HD void xyzzw_add_mixed_os(XyzzW &acc, const AffW &q, bool neg_q) {
    if (is_inf(acc)) { acc.x = q.x; acc.y = neg_q ? neg2(q.y) : q.y; acc.zz = w_one<FqW>(); acc.zzz = w_one<FqW>(); return; }
    const FqW9 u2 = LM(q.x, acc.zz), s2 = LM(q.y, acc.zzz);
    const FqW9 p = sub6(u2, acc.x);
    FqW9 r;
    {
        const uint32_t m = neg_q ? 0xffffffffu : 0u;
#pragma unroll
        for (int i = 0; i < 9; i++) r.l[i] = FqW::PAD8[i] - acc.y.l[i] + ((s2.l[i] ^ m) - m);
        r = normw(r);
    }
    if (maybe_zero_mod_p(p)) { xyzzw_add_mixed_special(acc, q, neg_q, p, r); return; }       // P == +-Q: rare
    const FqW9 pp = LS(p), rr = LS(r), ppp = LM(p, pp), qq = LM(acc.x, pp);
    FqW9 x3;
#pragma unroll
    for (int i = 0; i < 9; i++) x3.l[i] = rr.l[i] + FqW::PAD4[i] - ppp.l[i] - 2 * qq.l[i];
    x3 = normw(x3);
    const FqW9 zz3 = LM(acc.zz, pp), zzz3 = LM(acc.zzz, ppp);
    acc.y = LMA(r, sub6(qq, x3), acc.y, neg2(ppp));           // R*(Q - X3) - Y*PPP, one reduction
    acc.x = x3; acc.zz = zz3; acc.zzz = zzz3;
}
constexpr size_t G1NTT_LDS_ISO = (size_t)G1NTT_TABLE * 18 * G1NTT_THREADS * sizeof(uint32_t);   // 73728 B
__device__ __forceinline__ void lds_put_aff(uint32_t *tab, int e, const FqW9 &x, const FqW9 &y) {
#pragma unroll
    for (int k = 0; k < 9; k++) { tab[(e * 18 + k) * G1NTT_THREADS + threadIdx.x] = x.l[k]; tab[(e * 18 + 9 + k) * G1NTT_THREADS + threadIdx.x] = y.l[k]; }
}
__device__ __forceinline__ AffW lds_get_aff(const uint32_t *tab, int e) {
    AffW q;
#pragma unroll
    for (int k = 0; k < 9; k++) { q.x.l[k] = tab[(e * 18 + k) * G1NTT_THREADS + threadIdx.x]; q.y.l[k] = tab[(e * 18 + 9 + k) * G1NTT_THREADS + threadIdx.x]; }
    return q;
}
__device__ __forceinline__ XyzzW g1_mul_scalar_iso(const XyzzW &b, const Fr &k, uint32_t *tab) {
    if (is_inf(b)) return xyzzw_identity();
    FqW9 dzz, dzzz;
    {   // table: b, 2b, 3b, 4b over one denominator pair
        XyzzW t1 = b, t2 = b;
        g1_double_call(&t2);
        XyzzW t3 = t2; g1_add_call(&t3, &b);
        XyzzW t4 = t2; g1_double_call(&t4);
        {
            const FqW9 p12 = LM(t1.zz, t2.zz), p34 = LM(t3.zz, t4.zz);
            t1.x = LM(t1.x, LM(t2.zz, p34)); t2.x = LM(t2.x, LM(t1.zz, p34)); t3.x = LM(t3.x, LM(p12, t4.zz)); t4.x = LM(t4.x, LM(p12, t3.zz));
            dzz = LM(p12, p34);
        }
        {
            const FqW9 p12 = LM(t1.zzz, t2.zzz), p34 = LM(t3.zzz, t4.zzz);
            t1.y = LM(t1.y, LM(t2.zzz, p34)); t2.y = LM(t2.y, LM(t1.zzz, p34)); t3.y = LM(t3.y, LM(p12, t4.zzz)); t4.y = LM(t4.y, LM(p12, t3.zzz));
            dzzz = LM(p12, p34);
        }
        lds_put_aff(tab, 0, t1.x, t1.y); lds_put_aff(tab, 1, t2.x, t2.y); lds_put_aff(tab, 2, t3.x, t3.y); lds_put_aff(tab, 3, t4.x, t4.y);
    }
    uint32_t dig[2][6];
    uint32_t flip[2];
    {
        const GlvSplit sp = glv_split(k.l);
        glv_digits(sp.k1, dig[0]);
        glv_digits(sp.k2, dig[1]);
        flip[0] = sp.neg1 ? 8u : 0u; flip[1] = sp.neg2 ? 8u : 0u;
    }
    FqW9 beta;
#pragma unroll
    for (int i = 0; i < 9; i++) beta.l[i] = glv::BETA_W[i];
    XyzzW acc = xyzzw_identity();
    for (int w = 42; w >= 0; w--) {
        for (int r = 0; r < 3; r++) acc = xyzzw_double(acc);      // one inlined doubling site (identity passes through)
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            const uint32_t code = ((dig[h][w >> 3] >> (4 * (w & 7))) & 15u), mag = code & 7u;
            if (mag) {
                AffW q = lds_get_aff(tab, (int)mag - 1);
                if (h) q.x = LM(q.x, beta);                        // phi: x -> beta x (the scaling commutes with it)
                xyzzw_add_mixed_os(acc, q, ((code ^ flip[h]) & 8u) != 0);     // the one inlined mixed-addition site
            }
        }
    }
    acc.zz = LM(acc.zz, dzz); acc.zzz = LM(acc.zzz, dzzz);       // back from the isomorphic curve (the identity stays the identity)
    return acc;
}

// ---- and with EIGHT effectively affine table points b .. 8b (the table entries are half as large now: the same 147 KB of LDS hold twice as many) and signed
// 4-bit windows: 128 doublings + 64 mixed additions + 32 products by beta + ~138 for the table = ~1960 field products (2400 in rounds 4-5, 2120 with four
// entries).  The eight points' X, Y wait in the LDS slots while the prefix / suffix products of their ZZ and ZZZ are formed in registers.
constexpr int G1NTT_TABLE8 = 8;
constexpr size_t G1NTT_LDS_ISO8 = (size_t)G1NTT_TABLE8 * 18 * G1NTT_THREADS * sizeof(uint32_t);   // 147456 B
__device__ __forceinline__ XyzzW g1_mul_scalar_iso8(const XyzzW &b, const Fr &k, uint32_t *tab) {
    if (is_inf(b)) return xyzzw_identity();
    FqW9 dzz, dzzz;
    {
        FqW9 zz[8], zzz[8];
        {   // b, 2b, .. 8b: X, Y to the LDS slots, ZZ / ZZZ stay
            XyzzW t[8];
            t[0] = b;
            t[1] = b; g1_double_call(&t[1]);
            t[2] = t[1]; g1_add_call(&t[2], &b);
            t[3] = t[1]; g1_double_call(&t[3]);
            t[4] = t[3]; g1_add_call(&t[4], &b);
            t[5] = t[2]; g1_double_call(&t[5]);
            t[6] = t[5]; g1_add_call(&t[6], &b);
            t[7] = t[3]; g1_double_call(&t[7]);
#pragma unroll
            for (int i = 0; i < 8; i++) { lds_put_aff(tab, i, t[i].x, t[i].y); zz[i] = t[i].zz; zzz[i] = t[i].zzz; }
        }
        // cofactor of entry i = product of the other seven: prefix * suffix; the X (Y) of the slot is scaled in place
        auto scale = [&](FqW9 (&z)[8], int off) __attribute__((always_inline)) -> FqW9 {
            FqW9 pre[8];                                          // pre[i] = z_0 .. z_{i-1}
            pre[1] = z[0];
#pragma unroll
            for (int i = 2; i < 8; i++) pre[i] = LM(pre[i - 1], z[i - 1]);
            FqW9 suf = z[7];                                      // z_{i+1} .. z_7 while walking down
            const FqW9 all = LM(pre[7], z[7]);
#pragma unroll
            for (int i = 7; i >= 0; i--) {
                FqW9 c;
                if (i == 7) c = pre[7]; else if (i == 0) c = suf; else c = LM(pre[i], suf);
                FqW9 v;
#pragma unroll
                for (int kk = 0; kk < 9; kk++) v.l[kk] = tab[(i * 18 + off + kk) * G1NTT_THREADS + threadIdx.x];
                v = LM(v, c);
#pragma unroll
                for (int kk = 0; kk < 9; kk++) tab[(i * 18 + off + kk) * G1NTT_THREADS + threadIdx.x] = v.l[kk];
                if (i > 0 && i < 7) suf = LM(suf, z[i]);
            }
            return all;
        };
        dzz = scale(zz, 0);
        dzzz = scale(zzz, 9);
    }
    uint32_t dig[2][6];
    uint32_t flip[2];
    {
        const GlvSplit sp = glv_split(k.l);
        glv_digits4(sp.k1, dig[0]);
        glv_digits4(sp.k2, dig[1]);
        flip[0] = sp.neg1 ? 16u : 0u; flip[1] = sp.neg2 ? 16u : 0u;
    }
    FqW9 beta;
#pragma unroll
    for (int i = 0; i < 9; i++) beta.l[i] = glv::BETA_W[i];
    XyzzW acc = xyzzw_identity();
    for (int w = 31; w >= 0; w--) {
        for (int r = 0; r < 4; r++) acc = xyzzw_double(acc);      // one inlined doubling site (identity passes through)
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            const uint32_t code = (dig[h][w / 6] >> (5 * (w % 6))) & 31u, mag = code & 15u;
            if (mag) {
                AffW q = lds_get_aff(tab, (int)mag - 1);
                if (h) q.x = LM(q.x, beta);                        // phi: x -> beta x (the scaling commutes with it)
                xyzzw_add_mixed_os(acc, q, ((code ^ flip[h]) & 16u) != 0);    // the one inlined mixed-addition site
            }
        }
    }
    acc.zz = LM(acc.zz, dzz); acc.zzz = LM(acc.zzz, dzzz);       // back from the isomorphic curve (the identity stays the identity)
    return acc;
}

}  // namespace plk
