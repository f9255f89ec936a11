// Fq12 on the device, in the flat representation of pairing.h — Fq[w]/(w^12 - 18 w^6 + 82) on field_dev.h's Fq — and the pairing product
// check e(A, Q0) e(B, Q1) == 1 from the line tables that plk_vk_load builds on the host (pairing.cpp miller_lines).  One check per lane.
// Everything is __host__ __device__: tests/host/fq12_dev_check.hip runs the same code on the CPU against pairing_product_is_one.
//
// The device never does twist arithmetic: a line of the Miller loop is l = -y_P + (m x_P) w + b w^3 with (m, b) in Fq2 tabulated per step,
// folded on upload to four Fq (m0 - 9 m1, m1, b0 - 9 b1, b1) so that l = c0 + c1 w + c3 w^3 + c7 w^7 + c9 w^9 costs two products.
//
// Final exponentiation.  Instead of the 2790-bit square-and-multiply of pairing.cpp (~4200 flat products) the lane decides the SAME
// predicate f^((p^12-1)/r) == 1 in ~330 products and without an inversion:
//   (p^12-1)/r = (p^6-1)(p^2+1) H,  H = (p^4-p^2+1)/r.   conj(x) = x^(p^6) is w -> -w (odd coefficients negated); its fixed field is Fq6,
//   the elements with even coefficients only.  With A = f^(p^2+1) = frob2(f) f:
//       f^((p^12-1)/r) = (conj(f)/f)^((p^2+1) H) = conj(A^H) / A^H,   which is 1 exactly when A^H lies in Fq6.
//   H = Hpos - Hneg with Hpos = p^3 + (6u^2+1) p^2 + p and Hneg = (36u^3+18u^2+12u) p + (36u^3+30u^2+18u+2)   (u = 4965661367192848881),
//   so A^H = X / Y with X = A^Hpos, Y = A^Hneg, from A^u, A^(u^2), A^(u^3) and Frobenius maps.  Y conj(Y) is in Fq6 and not zero, hence
//       X / Y in Fq6  <=>  X conj(Y) in Fq6  <=>  the six odd coefficients of X conj(Y) are zero.
//   f = 0 (no such Miller value exists for points on the curve) is answered "not one", as the host's exponentiation would.
// Frobenius: w^p = g w with g = xi^((p-1)/6) in Fq2 (host::frobenius_w, derived with fq2_pow at load time), so on z_k = a_k + b_k i, the Fq2
// coefficient of w^k (k < 6; flat c_k = a_k - 9 b_k, c_{k+6} = b_k):  frob1: z_k -> conj(z_k) g^k;  frob2: c_k -> c_k N(g)^k for all 12.
#pragma once
#include "ec_dev.h"

namespace plk {

struct Fq12D { Fq c[12]; };

// constants of one (Q0, Q1) pair: built on the host (verify_many.hip make_pairing_table), read-only on the device
struct PairingHead {
    Fq g1[5][2];            // g^k, k = 1..5, as (c0, c1) of Fq2
    Fq g2[11];              // N(g)^k, k = 1..11
    uint64_t ate_lo;        // host::ate_loop_lo()
    uint32_t lines;         // host::miller_line_count()
    uint32_t q_inf;         // bit j: Q_j is the point at infinity (its Miller loop is 1)
};
constexpr uint64_t BN_U = 4965661367192848881ULL;

PLK_HD Fq fq_x9(const Fq &a) { const Fq a8 = dbl(dbl(dbl(a))); return add(a8, a); }

// t[0..22] -> r, w^k = 18 w^(k-6) - 82 w^(k-12) from the top down
PLK_HD void fq12_reduce(Fq12D &r, Fq *t) {
#pragma unroll 1
    for (int k = 22; k >= 12; k--) {
        const Fq x2 = dbl(t[k]), x16 = dbl(dbl(dbl(x2))), x64 = dbl(dbl(x16));
        t[k - 6] = add(t[k - 6], add(x16, x2));
        t[k - 12] = sub(t[k - 12], add(add(x64, x16), x2));
    }
#pragma unroll 1
    for (int i = 0; i < 12; i++) r.c[i] = t[i];
}

PLK_HD void fq12_mul(Fq12D &r, const Fq12D &a, const Fq12D &b) {
    Fq t[23];
#pragma unroll 1
    for (int k = 0; k < 23; k++) t[k] = Fq::zero();
#pragma unroll 1
    for (int i = 0; i < 12; i++) {
        const Fq ai = a.c[i];
#pragma unroll 1
        for (int j = 0; j < 12; j++) t[i + j] = add(t[i + j], ECM(ai, b.c[j]));
    }
    fq12_reduce(r, t);
}

PLK_HD void fq12_sqr(Fq12D &r, const Fq12D &a) {
    Fq t[23];
#pragma unroll 1
    for (int k = 0; k < 23; k++) t[k] = Fq::zero();
#pragma unroll 1
    for (int i = 0; i < 12; i++) {
        const Fq ai = a.c[i], ai2 = dbl(ai);
        t[2 * i] = add(t[2 * i], ECM(ai, ai));
#pragma unroll 1
        for (int j = i + 1; j < 12; j++) t[i + j] = add(t[i + j], ECM(ai2, a.c[j]));
    }
    fq12_reduce(r, t);
}

// f *= c0 + c1 w + c3 w^3 + c7 w^7 + c9 w^9   (60 products instead of 144)
PLK_HD void fq12_mul_line(Fq12D &f, const Fq &c0, const Fq &c1, const Fq &c3, const Fq &c7, const Fq &c9) {
    Fq t[23];
#pragma unroll 1
    for (int k = 0; k < 23; k++) t[k] = Fq::zero();
#pragma unroll 1
    for (int i = 0; i < 12; i++) {
        const Fq ai = f.c[i];
        t[i] = add(t[i], ECM(ai, c0));
        t[i + 1] = add(t[i + 1], ECM(ai, c1));
        t[i + 3] = add(t[i + 3], ECM(ai, c3));
        t[i + 7] = add(t[i + 7], ECM(ai, c7));
        t[i + 9] = add(t[i + 9], ECM(ai, c9));
    }
    fq12_reduce(f, t);
}

PLK_HD void fq12_conj(Fq12D &r, const Fq12D &a) {
#pragma unroll 1
    for (int i = 0; i < 12; i++) r.c[i] = (i & 1) ? neg(a.c[i]) : a.c[i];
}

PLK_HD void fq12_frob2(Fq12D &r, const Fq12D &a, const PairingHead *h) {
    r.c[0] = a.c[0];
#pragma unroll 1
    for (int k = 1; k < 12; k++) r.c[k] = ECM(a.c[k], h->g2[k - 1]);
}

PLK_HD void fq12_frob1(Fq12D &r, const Fq12D &a, const PairingHead *h) {
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
        Fq z0 = add(a.c[k], fq_x9(a.c[k + 6])), z1 = neg(a.c[k + 6]);          // conj(a_k + b_k i)
        if (k) {
            const Fq g0 = h->g1[k - 1][0], g1 = h->g1[k - 1][1];
            const Fq n0 = sub(ECM(z0, g0), ECM(z1, g1)), n1 = add(ECM(z0, g1), ECM(z1, g0));
            z0 = n0; z1 = n1;
        }
        r.c[k] = sub(z0, fq_x9(z1));
        r.c[k + 6] = z1;
    }
}

// a^e, e > 0, square-and-multiply from the top bit
PLK_HD void fq12_pow(Fq12D &r, const Fq12D &a, uint64_t e) {
    int top = 63;
    while (!((e >> top) & 1)) top--;
    Fq12D acc = a;
#pragma unroll 1
    for (int i = top - 1; i >= 0; i--) {
        fq12_sqr(acc, acc);
        if ((e >> i) & 1) fq12_mul(acc, acc, a);
    }
    r = acc;
}

PLK_HD bool fq_on_curve(const Fq &x, const Fq &y) {
    if (x.is_zero() && y.is_zero()) return true;
    return ECM(y, y) == add(ECM(ECM(x, x), x), from_u64<FqParams>(3));
}

// e(A, Q0) e(B, Q1) == 1 ?   lines: per step j and point q the four folded Fq at lines[(j * 2 + q) * 4 ..]; A, B on the curve (or infinity)
PLK_HD bool pairing_is_one_from_lines(const Fq &ax, const Fq &ay, const Fq &bx, const Fq &by, const PairingHead *h, const Fq *lines) {
    const bool on[2] = {!(ax.is_zero() && ay.is_zero()) && !(h->q_inf & 1u), !(bx.is_zero() && by.is_zero()) && !(h->q_inf & 2u)};
    const Fq px[2] = {ax, bx}, ny[2] = {neg(ay), neg(by)};
    Fq12D f;
#pragma unroll 1
    for (int i = 0; i < 12; i++) f.c[i] = Fq::zero();
    f.c[0] = Fq::one();
    if (on[0] || on[1]) {
        uint32_t k = 0;
        auto step = [&]() {
#pragma unroll 1
            for (int q = 0; q < 2; q++) {
                if (!on[q]) continue;
                const Fq *l = lines + ((size_t)k * 2 + q) * 4;
                fq12_mul_line(f, ny[q], ECM(l[0], px[q]), l[2], ECM(l[1], px[q]), l[3]);
            }
            k++;
        };
#pragma unroll 1
        for (int i = 63; i >= 0; i--) {
            fq12_sqr(f, f);
            step();
            if ((h->ate_lo >> i) & 1) step();
        }
        step(); step();
    }
    {
        uint32_t nz = 0;
#pragma unroll 1
        for (int i = 0; i < 12; i++) nz |= f.c[i].is_zero() ? 0u : 1u;
        if (!nz) return false;
    }
    Fq12D A, t;
    fq12_frob2(t, f, h);
    fq12_mul(A, t, f);                                              // f^(p^2+1)
    Fq12D au, au2, au3;
    fq12_pow(au, A, BN_U); fq12_pow(au2, au, BN_U); fq12_pow(au3, au2, BN_U);
    Fq12D X, Y;
    {   // X = frob3(A) frob2(A^(6u^2+1)) frob1(A)
        Fq12D f1, f3, s2;
        fq12_frob1(f1, A, h);
        fq12_frob2(f3, f1, h);                                      // A^(p^3)
        fq12_pow(s2, au2, 6); fq12_mul(s2, s2, A); fq12_frob2(s2, s2, h);   // (A^(6u^2+1))^(p^2)
        fq12_mul(X, f3, s2); fq12_mul(X, X, f1);
    }
    {   // Y = frob1(A^(36u^3+18u^2+12u)) A^(36u^3+30u^2+18u+2)
        Fq12D t36, y1, y0, s;
        fq12_pow(t36, au3, 36);
        fq12_pow(s, au2, 18); fq12_mul(y1, t36, s);
        fq12_pow(s, au, 12); fq12_mul(y1, y1, s);
        fq12_frob1(y1, y1, h);
        fq12_pow(s, au2, 30); fq12_mul(y0, t36, s);
        fq12_pow(s, au, 18); fq12_mul(y0, y0, s);
        fq12_sqr(s, A); fq12_mul(y0, y0, s);
        fq12_mul(Y, y1, y0);
    }
    fq12_conj(Y, Y);
    fq12_mul(t, X, Y);
    uint32_t odd = 0;
#pragma unroll 1
    for (int i = 1; i < 12; i += 2) odd |= t.c[i].is_zero() ? 0u : 1u;
    return odd == 0;
}

}  // namespace plk
