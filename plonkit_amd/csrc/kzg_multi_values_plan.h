// The multi-point openings from VALUES ON THE DOMAIN (kzg_multi_values.hip): the host scalar algebra around the kernels, as plain functions
// over HFr.  Host only, like kzg_multi_plan.h, whose weights, matrix, c_i and r_i(u) it calls and does not repeat; a stand-alone program
// holds it against the Python-integer model (tests/host/kzg_multi_values_plan_check.cpp, tests/gen/kzg_multi_values_cases.py).
// NO COUNTERPART IN THE REFERENCE.
//
// N = 2^log_n, omega the N-th root of the domain, f[x] = f(omega^x), d_xj = omega^x - t_j.  A point is ON THE DOMAIN when t^N = 1
// (t = omega^k; the kernel that forms the denominators reports k).  With b_xj = omega^x / d_xj:
//     evaluation         f(t_j) = -(t_j^N - 1) / N * sum_x f[x] b_xj                       off the domain (barycentric), f[k_j] on it
//     one term of D_t    D_{t_j}[G][x] = (G[x] - G(t_j)) / d_xj                            x != k_j
//                        D_{t_j}[G][k_j] = -1 / t_j * sum_{x != k_j} (G[x] - G(t_j)) b_xj  the value there of the polynomial quotient
// The sum at k_j is linear in G, so it needs only the sums S_ij = sum_{x != k_j} f_i[x] b_xj that the evaluation pass forms anyway, and
//     sum_{x != k} omega^x / (omega^x - omega^k) = sum_{m = 1}^{N-1} 1 / (1 - omega^-m) = (N - 1) / 2
// (pair m with N - m: 1 / (1 - z) + 1 / (1 - 1/z) = 1), a constant of the size alone.
// The second quotient is D_u[sum_i c_i f_i - Z_T(u) h]: L = sum_i c_i (f_i - r_i(u)) - Z_T(u) h vanishes at u, so the value the operator
// subtracts is sum_i c_i r_i(u), known from the evaluations: no evaluation pass over h.
#pragma once
#include "kzg_multi_plan.h"

namespace plk {
namespace host {

constexpr uint32_t KML_NONE = 0xffffffffu;           // "not on the domain" where an index k is expected
constexpr uint32_t KML_GROUP = 32;                   // polynomials per launch of the sums kernel: 32 x 8 pairs, a lane each
constexpr uint32_t KML_SUB = 256;                    // elements whose b_xj one workgroup holds in LDS at a time
static_assert(KML_GROUP * KM_MAX_POINTS == KM_THREADS && KML_SUB == KM_THREADS && KM_TILE % KML_SUB == 0, "a lane per pair, a lane per element");

inline bool kml_on_domain(const HFr &t, uint32_t log_n) { return t.pow_u64(1ull << log_n) == HFr::one(); }
// -(t^N - 1) / N: what turns sum_x f[x] omega^x / (omega^x - t) into f(t)
inline HFr kml_eval_scale(const HFr &t, uint32_t log_n) { return -((t.pow_u64(1ull << log_n) - HFr::one()) * HFr::from_u64(1ull << log_n).inv()); }
// (N - 1) / 2 = sum_{x != k} omega^x / (omega^x - omega^k)
inline HFr kml_rest_sum(uint32_t log_n) { return HFr::from_u64((1ull << log_n) - 1) * HFr::from_u64(2).inv(); }
// how many lanes share one pair in the sums kernel (each takes every slices-th element)
inline uint32_t kml_slices(uint32_t pairs) { return KM_THREADS / pairs; }

// g[j] = G_j(t_j) = sum_i m[i * npoints + j] y[i * npoints + j]: the value D_{t_j} subtracts (entries outside the sets are zero in m)
inline void kml_g(const HFr *m, const HFr *y, uint32_t count, uint32_t npoints, HFr *g) {
    for (uint32_t j = 0; j < npoints; j++) {
        g[j] = HFr::zero();
        for (uint32_t i = 0; i < count; i++) if (!m[i * npoints + j].is_zero()) g[j] = g[j] + m[i * npoints + j] * y[i * npoints + j];
    }
}
// D_t[G][k] for t = omega^k from ms = sum_i m_i S_i, S_i = sum_{x != k} f_i[x] omega^x / (omega^x - t), and g = G(t)
inline HFr kml_at_domain_point(const HFr &t, const HFr &ms, const HFr &g, uint32_t log_n) { return -((ms - g * kml_rest_sum(log_n)) * t.inv()); }

// sum_i c_i r_i(u): the value at u of sum_i c_i f_i - Z_T(u) h.  w and y are the count x npoints weights and evaluations.
inline HFr kml_value_at_u(const HFr *points, uint32_t npoints, const uint32_t *sets, uint32_t count, const HFr *c, const HFr *w, const HFr *y, const HFr &u) {
    HFr v = HFr::zero();
    for (uint32_t i = 0; i < count; i++) v = v + c[i] * km_r_at(points, npoints, sets[i], w + i * npoints, y + i * npoints, u);
    return v;
}

}  // namespace host
}  // namespace plk
