// Host side of fq12_dev.h: the constants and the folded line table of one (Q0, Q1) pair, built with pairing.cpp's own steps.
// Used by plk_vk_load / plk_pairing_check_many_dev (verify_many.hip) and by tests/host/fq12_dev_check.hip.
#pragma once
#include <vector>
#include "fq12_dev.h"
#include "pairing.h"

namespace plk {

inline Fq fq_of(const host::HFq &a) { Fq r; memcpy(r.l, a.l, 32); return r; }          // the same Montgomery limbs (hostmath.h)

// lines: miller_line_count() steps x 2 points x 4 Fq = (m0 - 9 m1, m1, b0 - 9 b1, b1); a point at infinity leaves zeros and its bit in q_inf
inline void make_pairing_table(const host::G2Affine g2[2], PairingHead *head, std::vector<Fq> *lines) {
    using namespace host;
    const HFq nine = HFq::from_u64(9);
    const Fq2 g = frobenius_w();
    const HFq ng = g.c0.sqr() + g.c1.sqr();                        // N(g) = g conj(g): w^(p^2) = N(g) w
    Fq2 gk = Fq2::one(); HFq nk = HFq::one();
    for (int k = 1; k <= 11; k++) {
        gk = gk * g; nk = nk * ng;
        if (k <= 5) { head->g1[k - 1][0] = fq_of(gk.c0); head->g1[k - 1][1] = fq_of(gk.c1); }
        head->g2[k - 1] = fq_of(nk);
    }
    const int n = miller_line_count();
    head->ate_lo = ate_loop_lo(); head->lines = (uint32_t)n; head->q_inf = 0;
    lines->assign((size_t)n * 8, Fq::zero());
    std::vector<Fq2> raw((size_t)2 * n);
    for (int q = 0; q < 2; q++) {
        if (g2[q].inf) { head->q_inf |= 1u << q; continue; }
        miller_lines(g2[q], raw.data());
        for (int k = 0; k < n; k++) {
            const Fq2 &m = raw[2 * k], &b = raw[2 * k + 1];
            Fq *o = lines->data() + ((size_t)k * 2 + q) * 4;
            o[0] = fq_of(m.c0 - m.c1 * nine); o[1] = fq_of(m.c1); o[2] = fq_of(b.c0 - b.c1 * nine); o[3] = fq_of(b.c1);
        }
    }
}

}  // namespace plk
