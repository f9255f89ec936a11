// The multi-point openings of kzg_multi.hip FROM VALUES ON THE DOMAIN: no inverse transform, no coefficient copies.  The same evaluations, u,
// W and W' as plk_kzg_open_multi_dev gives for the coefficients of the same polynomials, committed against the Lagrange-form key.
// Contracts: include/plonkit_amd.h; the algebra: kzg_multi_values_plan.h (and kzg_multi_plan.h behind it).  NO COUNTERPART IN THE REFERENCE.
//
// In values every step is point-wise or a reduction.  With d_xj = omega^x - t_j (1 where it vanishes: t_j = omega^k_j, decided on the
// host by t_j^N = 1 and reported by the lane that owns k_j) and P_x = prod_j d_xj:
//   k_kml_denoms<NP>    A[x] = B[x] = W(P_x), canonical
//   scan_pair_mult      A <- exclusive prefix products, B <- exclusive suffix products, block-local (poly.hip); ONE host inversion of the total
//   k_kml_sums<NP>      S_ij = sum_{x != k_j} f_i[x] omega^x / d_xj for the pairs (i, j) of the sets, per tile of 2048 elements.  Per 256
//                       elements the workgroup works in two shapes: a lane per ELEMENT forms 1 / P_x = A B (block prefixes) / total, the
//                       cofactors prod_{l != j} d_xl from prefix and suffix products in registers, and leaves b_xj = omega^x / d_xj in
//                       LDS (NP x 8 KiB); then a lane per PAIR walks the 256 elements, its polynomial against its point's row.  The
//                       denominators cost 4 + 4 NP products per element whatever the number of polynomials, a pair costs one product per
//                       element, and the loads of a wave's pairs fall into the lines its neighbours have just fetched (products, not
//                       bytes, bound this kernel).  Fewer than 129 pairs: 256 / pairs lanes share a pair, every slices-th element each.
//   k_kml_sum_finish    the tiles' partial sums, and f_i[k_j] for the points on the domain
//   k_kml_quot<NP>      out[x] = sum_j (G_j[x] - g_j) / d_xj, G_j = sum_i coef_ij f_i: a lane per element, element order
//                       block * 2048 + e * 256 + tid (no chain along the index: every load of a wave is 2 KiB of whole lines); each
//                       polynomial is read once for all points, `out` is written once; at x = k_j term j is the host's value
//                       (kml_at_domain_point), the other terms are ordinary.  out may be one of the inputs: a lane reads position x of
//                       every input before it writes position x, and no other lane touches x.
// Working memory: A, B, the output vector, pairs x tiles partial sums; nothing grows with the number of polynomials.
// Domains (kzg.hip): vectors and sums carry 2^256 (E); the scans, the omega table, the points and the matrix live in the 2^261 domain (W); a
// product of the 29-bit layer removes 2^261, so W x W = W and W x E = E.
// Bounds: a product is below 1.03 p + (left operand) / 170.  k_kml_sums reduces its accumulator after every 32 products (< 34 p; reduce_small
// takes 64 p).  k_kml_quot: G_j gathers at most 64 products and -g_j (< 68 p of the layer's 170 p), normalised after every addition; the sum
// of the 8 terms and the host's values stays below 20 p.
#include "ctx.h"
#include "msm.h"
#include "poly.h"
#include "ntt.h"
#include "field29_dev.h"
#include "prover_math.h"
#include "kzg_multi_values_plan.h"
#include "kzg_scratch.h"
#include <cstring>
#include <string>
#include <vector>

namespace plk {

using host::KM_MAX_POLYS; using host::KM_MAX_OPEN; using host::KM_MAX_POINTS; using host::KM_TILE; using host::KM_THREADS; using host::KM_EPT;
using host::KML_NONE; using host::KML_GROUP; using host::KML_SUB;
static_assert(KM_TILE == POLY_SCAN_BLOCK && KM_TILE == KM_THREADS * KM_EPT, "the consumers fold in the scan's block prefixes: same block size");

// what every kernel needs of one prepared set of points
struct KmlPlanDev {
    const Fr *A, *B, *preA, *preB;      // the two scans and their block prefixes in scan order (null: one block)
    Fr s_w;                             // W(1 / prod_x P_x)
    Fr t_w[KM_MAX_POINTS];              // W(t_j), canonical
    uint32_t k[KM_MAX_POINTS];          // t_j = omega^k[j], or KML_NONE
    PowTable tw;                        // the omega table, W
    uint32_t n, nb, shift, npoints;
};
struct KmlSumArgs {
    const Fr *f[KML_GROUP];
    uint8_t pi[KM_THREADS], pj[KM_THREADS];   // pair -> polynomial of this launch, point
    uint32_t pairs, slices;
    Fr *partials;                       // pairs x nb (E, canonical)
};
struct KmlQuotArgs {
    const Fr *f[KM_MAX_POLYS];
    uint8_t nz[KM_MAX_POLYS];           // bit j: coef[i][j] is not zero
    uint32_t count;
    const Fr *cst;                      // device: KM_MAX_POINTS x -G_j(t_j) (E) | KM_MAX_POINTS x D_{t_j}[G_j][k_j] for the points on the domain (E) |
                                        // the matrix, count x KM_MAX_POINTS (W).  (In memory, not in the arguments: 16 more scalars held in
                                        // registers beside the points made k_kml_quot<8> spill.)
    Fr *out;
};

__device__ __forceinline__ FrW9 kml_ldw(const Fr *p) { return unpack<FrW>(load_fp(p)); }
__device__ __forceinline__ FrW9 kml_omega(const PowTable &t, uint32_t e) { return mulw(kml_ldw(t.lo + (e & (POW_TAB - 1))), kml_ldw(t.hi + (e >> POW_SPLIT))); }
// W(1 / total) with the prefixes of block `blk` of both scans folded in: 1 / P_x = A[x] B[x] times this
__device__ __forceinline__ FrW9 kml_block_scale(const KmlPlanDev &p, uint32_t blk) {
    FrW9 c = unpack<FrW>(p.s_w);
    if (p.preA) c = mulw(mulw(kml_ldw(p.preA + blk), kml_ldw(p.preB + (p.nb - 1 - blk))), c);
    return c;
}
// q[j] = prod_{l != j} d_xl, d_xl = omega^x - t_l (1 where it vanishes and for l >= npoints); NP = 1: nothing to do, q is not read
template <int NP>
__device__ __forceinline__ void kml_cofactors(const KmlPlanDev &p, const FrW9 &om, uint32_t x, FrW9 (&q)[NP]) {
    if constexpr (NP > 1) {
        FrW9 d[NP];
        static_for<NP>([&](auto J) {
            constexpr int j = decltype(J)::value;
            d[j] = ((uint32_t)j < p.npoints && x != p.k[j]) ? sub2(om, unpack<FrW>(p.t_w[j])) : w_one<FrW>();
        });
        q[1] = d[0];
        static_for<NP - 2>([&](auto J) { constexpr int j = decltype(J)::value + 2; q[j] = mulw(q[j - 1], d[j - 1]); });      // prefixes
        FrW9 suf = d[NP - 1];
        static_for<NP - 1>([&](auto J) {                                                                                  // suffixes, from the top
            constexpr int j = NP - 2 - decltype(J)::value;
            if constexpr (j == 0) q[0] = suf;
            else { q[j] = mulw(q[j], suf); suf = mulw(suf, d[j]); }
        });
    }
}

// a[x] = b[x] = W(P_x), canonical; the lane whose factor j vanishes takes 1 for it and reports x as k_out[j]
template <int NP>
__global__ void __launch_bounds__(KM_THREADS) k_kml_denoms(Fr *a, Fr *b, KmlPlanDev p, uint32_t *k_out) {
    const uint32_t x = blockIdx.x * KM_THREADS + threadIdx.x;
    if (x >= p.n) return;
    const FrW9 om = kml_omega(p.tw, x << p.shift);
    FrW9 P = w_one<FrW>();
    static_for<NP>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if ((uint32_t)j < p.npoints) {
            FrW9 d = reduce_small(sub2(om, unpack<FrW>(p.t_w[j])));
            if (w_all_zero(d)) { d = w_one<FrW>(); k_out[j] = x; }
            P = j == 0 ? d : mulw(P, d);
        }
    });
    const Fr v = pack<FrParams>(csub_p(P));
    store_fp(a + x, v);
    store_fp(b + x, v);
}

template <int NP>
__global__ void __launch_bounds__(KM_THREADS) k_kml_sums(KmlSumArgs a, KmlPlanDev p) {
    __shared__ __attribute__((aligned(16))) Fr sh[NP * KML_SUB];    // row j: b_xj of the 256 elements in hand (W, canonical); at the end the lanes' sums
    const uint32_t tid = threadIdx.x, blk = blockIdx.x;
    const FrW9 scale = kml_block_scale(p, blk);
    // the lane's pair
    const bool busy = tid < a.pairs * a.slices;
    const uint32_t pair = busy ? tid % a.pairs : 0, slice = busy ? tid / a.pairs : 0;
    const uint32_t pj = a.pj[pair], skip = p.k[pj];
    const Fr *f = a.f[a.pi[pair]];
    const Fr *row = sh + pj * KML_SUB;
    FrW9 acc = w_zero<FrW>();
    uint32_t gathered = 0;
#pragma unroll 1
    for (uint32_t e = 0; e < KM_EPT; e++) {
        const uint32_t x0 = blk * KM_TILE + e * KML_SUB, x = x0 + tid;
        if (x0 >= p.n) break;                                     // (uniform: a size below one tile)
        if (x < p.n) {
            const FrW9 om = kml_omega(p.tw, x << p.shift);
            FrW9 q[NP];
            kml_cofactors<NP>(p, om, x, q);
            const FrW9 b = mulw(mulw(mulw(kml_ldw(p.A + x), kml_ldw(p.B + x)), scale), om);           // omega^x / P_x
            static_for<NP>([&](auto J) {
                constexpr int j = decltype(J)::value;
                sh[j * KML_SUB + tid] = pack<FrParams>(csub_p(NP == 1 ? b : mulw(q[j], b)));
            });
        }
        __syncthreads();
        if (busy) {
            const uint32_t end = p.n - x0 < KML_SUB ? p.n - x0 : KML_SUB;
#pragma unroll 1
            for (uint32_t xx = slice; xx < end; xx += a.slices) {
                if (x0 + xx == skip) continue;
                acc = addn(acc, mulw(kml_ldw(f + x0 + xx), unpack<FrW>(row[xx])));
                if ((++gathered & 31u) == 0) acc = reduce_small(acc);
            }
        }
        __syncthreads();
    }
    sh[tid] = pack<FrParams>(reduce_small(acc));
    __syncthreads();
    if (tid < a.pairs) {
        Fr s = sh[tid];
        for (uint32_t k = 1; k < a.slices; k++) s = add(s, sh[tid + k * a.pairs]);
        store_fp(a.partials + (size_t)tid * p.nb + blk, s);
    }
}

// results[pair] = the sum of the pair's partials; results[pairs + pair] = f_i[k_j] for a point on the domain, zero otherwise
__global__ void __launch_bounds__(KM_THREADS) k_kml_sum_finish(Fr *results, KmlSumArgs a, KmlPlanDev p) {
    __shared__ __attribute__((aligned(16))) Fr sh[KM_THREADS];
    const uint32_t tid = threadIdx.x, pair = blockIdx.x;
    Fr acc = Fr::zero();
    for (uint32_t b = tid; b < p.nb; b += KM_THREADS) acc = add(acc, load_fp(a.partials + (size_t)pair * p.nb + b));
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t off = KM_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) { acc = add(acc, sh[tid + off]); sh[tid] = acc; }
        __syncthreads();
    }
    if (tid == 0) {
        store_fp(results + pair, acc);
        const uint32_t k = p.k[a.pj[pair]];
        store_fp(results + a.pairs + pair, k != KML_NONE ? load_fp(a.f[a.pi[pair]] + k) : Fr::zero());
    }
}

template <int NP>
__global__ void __launch_bounds__(KM_THREADS) k_kml_quot(KmlQuotArgs a, KmlPlanDev p) {
    const uint32_t tid = threadIdx.x, blk = blockIdx.x;
    const FrW9 scale = kml_block_scale(p, blk);
#pragma unroll 1
    for (uint32_t e = 0; e < KM_EPT; e++) {
        const uint32_t x = blk * KM_TILE + e * KM_THREADS + tid;
        if (x >= p.n) break;
        FrW9 q[NP], G[NP];
        kml_cofactors<NP>(p, kml_omega(p.tw, x << p.shift), x, q);
        const FrW9 ip = mulw(mulw(kml_ldw(p.A + x), kml_ldw(p.B + x)), scale);                       // 1 / P_x
        static_for<NP>([&](auto J) {                                                                 // q[j] <- 1 / d_xj
            constexpr int j = decltype(J)::value;
            q[j] = NP == 1 ? ip : mulw(q[j], ip);
            G[j] = kml_ldw(a.cst + j);
        });
#pragma unroll 1
        for (uint32_t i = 0; i < a.count; i++) {
            const uint32_t m = a.nz[i];
            if (!m) continue;
            const FrW9 v = kml_ldw(a.f[i] + x);
            static_for<NP>([&](auto J) {
                constexpr int j = decltype(J)::value;
                if ((m >> j) & 1) G[j] = addn(G[j], mulw(v, kml_ldw(a.cst + (2 + i) * KM_MAX_POINTS + j)));
            });
        }
        FrW9 h = w_zero<FrW>();
        static_for<NP>([&](auto J) {
            constexpr int j = decltype(J)::value;
            if ((uint32_t)j < p.npoints) h = addn(h, x == p.k[j] ? kml_ldw(a.cst + KM_MAX_POINTS + j) : mulw(G[j], q[j]));
        });
        store_fp(a.out + x, pack<FrParams>(reduce_small(h)));
    }
}

namespace {
using namespace host;

inline Fr kml_dev(const HFr &h) { Fr f; memcpy(f.l, h.l, 32); return f; }
inline HFr kml_host(const plk_fr *p) { HFr h; memcpy(h.l, p->l, 32); return h; }
inline bool kml_fr_ok(const plk_fr *p) { return !HFr::geq_p(p->l); }

#define KML_LAUNCH(KERNEL, np, grid, st, ...)                                                                          \
    do {                                                                                                               \
        if ((np) == 1) hipLaunchKernelGGL(KERNEL<1>, grid, dim3(KM_THREADS), 0, st, __VA_ARGS__);                       \
        else if ((np) == 2) hipLaunchKernelGGL(KERNEL<2>, grid, dim3(KM_THREADS), 0, st, __VA_ARGS__);                  \
        else if ((np) <= 4) hipLaunchKernelGGL(KERNEL<4>, grid, dim3(KM_THREADS), 0, st, __VA_ARGS__);                  \
        else hipLaunchKernelGGL(KERNEL<8>, grid, dim3(KM_THREADS), 0, st, __VA_ARGS__);                                 \
    } while (0)

// One prepared set of points.  Scratch: [k words | results | partials | A | B | the quotient's constants and matrix | extra]
struct KmlPlan {
    uint32_t log_n = 0, npoints = 0;
    HFr t[KM_MAX_POINTS];
    bool on_domain[KM_MAX_POINTS] = {};
    uint32_t *k_dev = nullptr;
    Fr *results = nullptr, *partials = nullptr, *coef = nullptr, *extra = nullptr;
    KmlPlanDev dev{};
    static size_t bytes(uint64_t n, uint64_t extra_elems) {
        const uint64_t nb = (n + KM_TILE - 1) / KM_TILE;
        return 256 + (size_t)(2 * KM_THREADS + KM_THREADS * nb + 2 * n + (2 + KM_MAX_POLYS) * KM_MAX_POINTS + extra_elems) * sizeof(Fr);
    }
};

// denominators, the two scans, the one inversion for all points.  Waits for `st` once.  A second plan of the same size and extra lies where
// the first one lay: what the caller keeps in `extra` survives it.
int32_t kml_prepare(plk_ctx *ctx, uint32_t log_n, const HFr *points, uint32_t npoints, uint64_t extra_elems, KzgScratch &ws, hipStream_t st, KmlPlan *out) {
    KmlPlan p;
    KmlPlanDev &d = p.dev;
    p.log_n = log_n; p.npoints = npoints;
    d.n = 1u << log_n; d.nb = (d.n + KM_TILE - 1) / KM_TILE; d.shift = MAX_LOG_N - log_n; d.npoints = npoints; d.tw = ctx->tw_fwd_w;
    PLK_TRY(ws.reserve(KmlPlan::bytes(d.n, extra_elems)));
    char *base = ctx->kzg_ws.as<char>();
    p.k_dev = reinterpret_cast<uint32_t *>(base);
    p.results = reinterpret_cast<Fr *>(base + 256);
    p.partials = p.results + 2 * KM_THREADS;
    Fr *A = p.partials + (size_t)KM_THREADS * d.nb, *B = A + d.n;
    p.coef = B + d.n;
    p.extra = p.coef + (2 + KM_MAX_POLYS) * KM_MAX_POINTS;
    for (uint32_t j = 0; j < KM_MAX_POINTS; j++) {
        p.t[j] = j < npoints ? points[j] : HFr::zero();
        p.on_domain[j] = j < npoints && kml_on_domain(points[j], log_n);
        d.t_w[j] = kml_dev(to_w(p.t[j]));
        d.k[j] = KML_NONE;
    }
    PLK_HIP(hipMemsetAsync(p.k_dev, 0xff, KM_MAX_POINTS * 4, st));
    KML_LAUNCH(k_kml_denoms, npoints, dim3((d.n + KM_THREADS - 1) / KM_THREADS), st, A, B, d, p.k_dev);
    PLK_HIP(hipGetLastError());
    const Fr *preA = nullptr, *preB = nullptr;
    PLK_TRY(scan_pair_mult(ctx, A, A, false, true, B, B, true, true, d.n, st, &preA, &preB));
    // the grand total: behind the block prefixes (canonical), or the one block's own total (lazily reduced)
    HFr total;
    PLK_HIP(hipMemcpyAsync(total.l, ctx->poly_tmp.as<Fr>() + (d.nb > 1 ? d.nb : 0), sizeof(Fr), hipMemcpyDeviceToHost, st));
    PLK_HIP(hipMemcpyAsync(d.k, p.k_dev, KM_MAX_POINTS * 4, hipMemcpyDeviceToHost, st));
    PLK_HIP(hipStreamSynchronize(st));
    if (HFr::geq_p(total.l)) HFr::sub_p(total.l);
    bool ok = !total.is_zero();
    for (uint32_t j = 0; j < KM_MAX_POINTS; j++) ok = ok && p.on_domain[j] == (d.k[j] != KML_NONE) && (d.k[j] == KML_NONE || d.k[j] < d.n);
    if (!ok) { set_error("kzg: the denominators of the values route are inconsistent"); return PLK_ERR_HIP; }
    // what was read is 32 * T in the external form: W(1 / T) = 32 * E(1 / T) = 32 * 32 * E(1 / (32 T))    (kzg.hip: values_prepare)
    d.A = A; d.B = B; d.preA = preA; d.preB = preB;
    d.s_w = kml_dev(to_w(to_w(total.inv())));
    *out = p;
    return PLK_OK;
}

// S[i * 8 + j] <- sum_{x != k_j} f_i[x] omega^x / (omega^x - t_j) and at_k[i * 8 + j] <- f_i[k_j] (points on the domain) for bit j of
// masks[i]; the other entries are left alone.  Groups of 32 polynomials, one launch each.  Waits.
int32_t kml_sums(const KmlPlan &p, const Fr *const *f, uint32_t count, const uint8_t *masks, HFr *S, HFr *at_k, hipStream_t st) {
    std::vector<HFr> got((size_t)2 * KM_THREADS * ((count + KML_GROUP - 1) / KML_GROUP));
    std::vector<KmlSumArgs> groups;
    for (uint32_t first = 0; first < count; first += KML_GROUP) {
        KmlSumArgs a{};
        const uint32_t m = count - first < KML_GROUP ? count - first : KML_GROUP;
        for (uint32_t i = 0; i < m; i++) {
            a.f[i] = f[first + i];
            for (uint32_t j = 0; j < p.npoints; j++) if ((masks[first + i] >> j) & 1) { a.pi[a.pairs] = (uint8_t)i; a.pj[a.pairs] = (uint8_t)j; a.pairs++; }
        }
        a.partials = p.partials;
        if (a.pairs) {
            a.slices = kml_slices(a.pairs);
            KML_LAUNCH(k_kml_sums, p.npoints, dim3(p.dev.nb), st, a, p.dev);
            hipLaunchKernelGGL(k_kml_sum_finish, dim3(a.pairs), dim3(KM_THREADS), 0, st, p.results, a, p.dev);
            PLK_HIP(hipGetLastError());
            PLK_HIP(hipMemcpyAsync(got.data() + (size_t)2 * KM_THREADS * groups.size(), p.results, (size_t)2 * a.pairs * sizeof(Fr), hipMemcpyDeviceToHost, st));
        }
        groups.push_back(a);
    }
    PLK_HIP(hipStreamSynchronize(st));
    for (size_t g = 0; g < groups.size(); g++) {
        const KmlSumArgs &a = groups[g];
        const HFr *r = got.data() + (size_t)2 * KM_THREADS * g;
        for (uint32_t k = 0; k < a.pairs; k++) {
            const size_t at = (g * KML_GROUP + a.pi[k]) * KM_MAX_POINTS + a.pj[k];
            S[at] = r[k];
            at_k[at] = r[a.pairs + k];
        }
    }
    return PLK_OK;
}

// y[i * npoints + j] = f_i(t_j) for bit j of masks[i], zero elsewhere: read on the domain, barycentric off it
void kml_evaluations(const KmlPlan &p, uint32_t count, const uint8_t *masks, const HFr *S, const HFr *at_k, HFr *y) {
    HFr scale[KM_MAX_POINTS];
    for (uint32_t j = 0; j < p.npoints; j++) scale[j] = kml_eval_scale(p.t[j], p.log_n);
    for (uint32_t i = 0; i < count; i++)
        for (uint32_t j = 0; j < p.npoints; j++) {
            const size_t at = (size_t)i * KM_MAX_POINTS + j;
            y[i * p.npoints + j] = !((masks[i] >> j) & 1) ? HFr::zero() : p.on_domain[j] ? at_k[at] : S[at] * scale[j];
        }
}

// out <- the values of sum_j D_{t_j}[sum_i coef[i * npoints + j] f_i] on st; g[j] = G_j(t_j); S as kml_sums left it (read for the points on
// the domain only).  `stage` is what the upload reads: the caller keeps it until the stream has been waited for.  out may be an input.
int32_t kml_quotient(const KmlPlan &p, const Fr *const *f, uint32_t count, const HFr *coef, const HFr *g, const HFr *S, Fr *out, std::vector<Fr> &stage, hipStream_t st) {
    KmlQuotArgs a{};
    a.count = count; a.cst = p.coef; a.out = out;
    stage.assign((size_t)(2 + count) * KM_MAX_POINTS, Fr::zero());
    for (uint32_t i = 0; i < count; i++) {
        a.f[i] = f[i];
        for (uint32_t j = 0; j < p.npoints; j++) {
            const HFr &v = coef[i * p.npoints + j];
            if (v.is_zero()) continue;
            a.nz[i] |= (uint8_t)(1u << j);
            stage[(size_t)(2 + i) * KM_MAX_POINTS + j] = kml_dev(to_w(v));
        }
    }
    for (uint32_t j = 0; j < p.npoints; j++) {
        stage[j] = kml_dev(-g[j]);
        if (!p.on_domain[j]) continue;
        HFr ms = HFr::zero();
        for (uint32_t i = 0; i < count; i++) if ((a.nz[i] >> j) & 1) ms = ms + coef[i * p.npoints + j] * S[(size_t)i * KM_MAX_POINTS + j];
        stage[KM_MAX_POINTS + j] = kml_dev(kml_at_domain_point(p.t[j], ms, g[j], p.log_n));
    }
    PLK_HIP(hipMemcpyAsync(p.coef, stage.data(), stage.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
    KML_LAUNCH(k_kml_quot, p.npoints, dim3(p.dev.nb), st, a, p.dev);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

uint8_t kml_mask_of_row(const HFr *row, uint32_t npoints) {
    uint8_t m = 0;
    for (uint32_t j = 0; j < npoints; j++) if (!row[j].is_zero()) m |= (uint8_t)(1u << j);
    return m;
}

int32_t open_multi_values(plk_ctx *ctx, const Fr *const *f, uint32_t count, uint32_t log_n, const HFr *points, uint32_t npoints, const uint32_t *sets, const HFr &gamma,
                          plk_kzg_challenge_fn challenge, void *user, plk_fr *evals, plk_fr *u_out, plk_g1_affine *proof, hipStream_t st) {
    const char *who = "plk_kzg_open_multi_values_dev";
    const uint64_t n = 1ull << log_n;
    HFr w[KM_MAX_OPEN * KM_MAX_POINTS], mat[KM_MAX_OPEN * KM_MAX_POINTS], y[KM_MAX_OPEN * KM_MAX_POINTS], g[KM_MAX_POINTS];
    std::vector<HFr> S((size_t)(KM_MAX_OPEN + 1) * KM_MAX_POINTS), at_k(S.size());
    km_weights(points, npoints, sets, count, w);
    km_matrix(w, gamma, count, npoints, mat);
    uint8_t masks[KM_MAX_OPEN + 1];
    for (uint32_t i = 0; i < count; i++) masks[i] = (uint8_t)sets[i];
    KzgScratch ws(ctx, st);
    StageTimer<6> ev;
    PLK_TRY(ev.start(ctx));
    PLK_TRY(ev.mark(0, st));
    // 1. one inversion for all points; y_ij = f_i(t_j) for j in S_i, every polynomial read once
    KmlPlan p;
    PLK_TRY(kml_prepare(ctx, log_n, points, npoints, n, ws, st, &p));
    Fr *h = p.extra;
    PLK_TRY(kml_sums(p, f, count, masks, S.data(), at_k.data(), st));
    kml_evaluations(p, count, masks, S.data(), at_k.data(), y);
    PLK_TRY(ev.mark(1, st));
    // 2. h = sum_j D_{t_j}[sum_i gamma^i w_ij f_i] in values, and W = commit(h) against the Lagrange-form key
    std::vector<Fr> stage1, stage2;
    kml_g(mat, y, count, npoints, g);
    PLK_TRY(kml_quotient(p, f, count, mat, g, S.data(), h, stage1, st));
    PLK_TRY(ev.mark(2, st));
    PLK_TRY(msm_commit(ctx, ctx->lagrange(), h, n, 0, &proof[0], st));   // waits
    PLK_TRY(ev.mark(3, st));
    for (uint32_t k = 0; k < count * npoints; k++) memcpy(evals[k].l, y[k].l, 32);
    // 3. the caller's challenge, once
    plk_fr u_raw;
    memset(&u_raw, 0, sizeof u_raw);
    const int32_t rc = challenge(user, &proof[0], &u_raw);
    if (rc != 0) { set_error(std::string(who) + ": the challenge callback returned " + std::to_string(rc)); return PLK_ERR_IO; }
    if (!kml_fr_ok(&u_raw)) { set_error(std::string(who) + ": the challenge callback gave a scalar that is not below r"); return PLK_ERR_ARG; }
    const HFr u = kml_host(&u_raw);
    *u_out = u_raw;
    // 4. W' = commit(D_u[sum_i c_i f_i - Z_T(u) h]): one point, the polynomials and h; the value at u is sum_i c_i r_i(u); written over h
    HFr c[KM_MAX_OPEN + 1], z_t;
    km_c(points, npoints, sets, count, gamma, u, c, &z_t);
    c[count] = -z_t;
    const HFr v = kml_value_at_u(points, npoints, sets, count, c, w, y, u);
    const Fr *f2[KM_MAX_OPEN + 1];
    for (uint32_t i = 0; i < count; i++) f2[i] = f[i];
    f2[count] = h;
    PLK_TRY(ev.mark(4, st));
    KmlPlan p2;
    PLK_TRY(kml_prepare(ctx, log_n, &u, 1, n, ws, st, &p2));
    if (p2.extra != h) { set_error(std::string(who) + ": the scratch moved between the two quotients"); return PLK_ERR_HIP; }
    if (p2.on_domain[0]) {                                         // u = omega^k: the identity above, held against the arrays at position k
        for (uint32_t i = 0; i <= count; i++) masks[i] = c[i].is_zero() ? 0 : 1;
        PLK_TRY(kml_sums(p2, f2, count + 1, masks, S.data(), at_k.data(), st));
        HFr at = HFr::zero();
        for (uint32_t i = 0; i <= count; i++) if (masks[i]) at = at + c[i] * at_k[(size_t)i * KM_MAX_POINTS];
        if (at != v) { set_error(std::string(who) + ": the second quotient's value at u = omega^" + std::to_string(p2.dev.k[0]) + " is inconsistent with the evaluations"); return PLK_ERR_HIP; }
    }
    PLK_TRY(kml_quotient(p2, f2, count + 1, c, &v, S.data(), h, stage2, st));
    PLK_TRY(msm_commit(ctx, ctx->lagrange(), h, n, 0, &proof[1], st));
    PLK_TRY(ev.mark(5, st));
    if (ev.on) {
        PLK_HIP(hipEventSynchronize(ev.e[5]));
        for (int k = 0; k < 3; k++) PLK_TRY(ev.elapsed(k, k + 1, &ctx->km_ms[k]));
        PLK_TRY(ev.elapsed(4, 5, &ctx->km_ms[3]));
        ctx->km_ms_valid = true;
    }
    return PLK_OK;
}

// what the three calls share: the size, the polynomials and the context (km_common's words), the points
int32_t kml_common(const char *who, plk_ctx *ctx, const void *const *values_dev, uint32_t count, uint32_t max_count, uint32_t log_n, const plk_fr *points, uint32_t npoints,
                   HFr *pts) {
    if (!points || log_n == 0 || log_n > MAX_LOG_N) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    PLK_TRY(km_common(who, ctx, values_dev, count, max_count, 1ull << log_n, npoints));
    for (uint32_t j = 0; j < npoints; j++) {
        if (!kml_fr_ok(points + j)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
        pts[j] = kml_host(points + j);
    }
    return PLK_OK;
}

}  // namespace
}  // namespace plk

using namespace plk;
using namespace plk::host;

extern "C" int32_t plk_poly_evaluate_values_multi_dev(plk_ctx *ctx, const void *const *values_dev, uint32_t count, uint32_t log_n, const plk_fr *points, uint32_t npoints,
                                                      const uint32_t *sets, plk_fr *evals, void *stream) {
    const char *who = "plk_poly_evaluate_values_multi_dev";
    if (!sets || !evals) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    HFr pts[KM_MAX_POINTS];
    PLK_TRY(kml_common(who, ctx, values_dev, count, KM_MAX_POLYS, log_n, points, npoints, pts));
    uint8_t masks[KM_MAX_POLYS];
    for (uint32_t i = 0; i < count; i++) {
        if (sets[i] >> npoints) { set_error(std::string(who) + ": " + km_sets_words(KM_SETS_BIT_ABOVE)); return PLK_ERR_ARG; }
        masks[i] = (uint8_t)sets[i];
    }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    try {
        KzgScratch ws(ctx, st);
        KmlPlan p;
        PLK_TRY(kml_prepare(ctx, log_n, pts, npoints, 0, ws, st, &p));
        std::vector<HFr> S((size_t)count * KM_MAX_POINTS), at_k(S.size()), y((size_t)count * npoints);
        PLK_TRY(kml_sums(p, reinterpret_cast<const Fr *const *>(values_dev), count, masks, S.data(), at_k.data(), st));
        kml_evaluations(p, count, masks, S.data(), at_k.data(), y.data());
        for (size_t k = 0; k < y.size(); k++) memcpy(evals[k].l, y[k].l, 32);
        return PLK_OK;
    } catch (const std::exception &e) { set_error(std::string(who) + ": " + e.what()); return PLK_ERR_HIP; }
}

extern "C" int32_t plk_poly_quotient_multi_values_dev(plk_ctx *ctx, const void *const *values_dev, uint32_t count, uint32_t log_n, const plk_fr *points, uint32_t npoints,
                                                      const plk_fr *coef, void *out_values_dev, void *stream) {
    const char *who = "plk_poly_quotient_multi_values_dev";
    if (!coef || !out_values_dev) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    HFr pts[KM_MAX_POINTS];
    PLK_TRY(kml_common(who, ctx, values_dev, count, KM_MAX_POLYS, log_n, points, npoints, pts));
    if ((uintptr_t)out_values_dev & 15u) { set_error(std::string(who) + ": device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    const uintptr_t span = ((uintptr_t)1 << log_n) * sizeof(Fr), o = (uintptr_t)out_values_dev;
    for (uint32_t i = 0; i < count; i++) {
        const uintptr_t q = (uintptr_t)values_dev[i];
        if (o < q + span && q < o + span) { set_error(std::string(who) + ": the output overlaps polynomial " + std::to_string(i)); return PLK_ERR_ARG; }
    }
    std::vector<HFr> cf((size_t)count * npoints);
    uint8_t masks[KM_MAX_POLYS];
    for (size_t k = 0; k < cf.size(); k++) {
        if (!kml_fr_ok(coef + k)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
        cf[k] = kml_host(coef + k);
    }
    for (uint32_t i = 0; i < count; i++) masks[i] = kml_mask_of_row(cf.data() + (size_t)i * npoints, npoints);
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    try {
        const Fr *const *f = reinterpret_cast<const Fr *const *>(values_dev);
        KzgScratch ws(ctx, st);
        KmlPlan p;
        PLK_TRY(kml_prepare(ctx, log_n, pts, npoints, 0, ws, st, &p));
        std::vector<HFr> S((size_t)count * KM_MAX_POINTS), at_k(S.size()), y((size_t)count * npoints);
        PLK_TRY(kml_sums(p, f, count, masks, S.data(), at_k.data(), st));        // the G_j(t_j), found here
        kml_evaluations(p, count, masks, S.data(), at_k.data(), y.data());
        HFr g[KM_MAX_POINTS];
        kml_g(cf.data(), y.data(), count, npoints, g);
        std::vector<Fr> stage;
        PLK_TRY(kml_quotient(p, f, count, cf.data(), g, S.data(), static_cast<Fr *>(out_values_dev), stage, st));
        PLK_HIP(hipStreamSynchronize(st));
        return PLK_OK;
    } catch (const std::exception &e) { set_error(std::string(who) + ": " + e.what()); return PLK_ERR_HIP; }
}

extern "C" int32_t plk_kzg_open_multi_values_dev(plk_ctx *ctx, const void *const *values_dev, uint32_t count, uint32_t log_n, const plk_fr *points, uint32_t npoints,
                                                 const uint32_t *sets, const plk_fr *gamma, plk_kzg_challenge_fn challenge, void *user, plk_fr *evals, plk_fr *u_out,
                                                 plk_g1_affine proof[2], void *stream) {
    const char *who = "plk_kzg_open_multi_values_dev";
    if (ctx) ctx->km_ms_valid = false;
    if (!sets || !gamma || !challenge || !evals || !u_out || !proof) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    HFr pts[KM_MAX_POINTS];
    PLK_TRY(kml_common(who, ctx, values_dev, count, KM_MAX_OPEN, log_n, points, npoints, pts));
    if (!kml_fr_ok(gamma)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
    const int verdict = km_check_sets(pts, npoints, sets, count);
    if (verdict != KM_SETS_OK) { set_error(std::string(who) + ": " + km_sets_words(verdict)); return PLK_ERR_ARG; }
    uint32_t l = 0;
    PLK_TRY(kzg_lagrange_key(ctx, 1ull << log_n, &l));
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    try {
        return open_multi_values(ctx, reinterpret_cast<const Fr *const *>(values_dev), count, log_n, pts, npoints, sets, kml_host(gamma), challenge, user, evals, u_out,
                                 proof, st);
    } catch (const std::exception &e) { set_error(std::string(who) + ": " + e.what()); return PLK_ERR_HIP; }
}
