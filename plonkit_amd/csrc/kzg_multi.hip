// Many polynomials at several points with a proof of two G1 points (Boneh-Drake-Fisch-Gabizon 2020, the scheme that needs only [tau]_2):
// the multi-point quotient kernels, the prover around them and the host verifier.  Contracts: include/plonkit_amd.h; the algebra and the
// identity that removes interpolation and long division: kzg_multi_plan.h.  NO COUNTERPART IN THE REFERENCE.
//
// THE QUOTIENT.  out[k] = sum_j H_j[k + 1] with H_j[l] = G_j[l] + t_j H_j[l + 1] (a Horner from the top, H_j[n] = 0) and
// G_j[l] = sum_i coef[i][j] f_i[l]: the sum over the points of (G_j - G_j(t_j)) / (x - t_j).  Tiles of 2048 coefficients, 8 per lane, the
// scan engine's shape (poly.h).  A lane keeps one accumulator per point on the 29-bit layer and walks its 8 coefficients downwards; each
// coefficient of each polynomial is loaded once and serves every point whose matrix entry is not zero.
// (One point, the shape of every second quotient: the lane forms G[l] for its 8 positions first, 256 consecutive bytes per polynomial.)
//   k_km_tiles<NP, false>  per tile and point the tile's Horner value sum_{l in tile} G_j[l] t_j^(l - l0)
//   k_km_carry             one workgroup per point: the value above each tile, C[q] = sum_{q' > q} V[q'] T^(q' - q - 1), T = t_j^2048, in place
//   k_km_tiles<NP, true>   re-reads the tile: the lane-local part of the sum goes to `out` during the walk, the lanes' Horner values are
//                          scanned across the tile (Kogge-Stone over LDS, step s multiplies by t_j^(8 * 2^s); the tile's carry enters at
//                          the last lane), and each lane adds t_j^(7 - e) times what stands above it.
// Every power is a per-call constant from the host (km_point_constants): no inverse, no per-element power, and t_j = 0 is an ordinary
// point (0^0 = 1 gives the shifted combination).  Traffic: (2 count + 1) x 32 n bytes plus the lane-local part written and read back
// by the lane that owns it (it stays in the cache between the two).
// Domains (poly.h): vectors carry 2^256 (E), constants 2^261 (W); a product of the layer removes 2^261, so W x E = E.
// Bounds: a product is below 1.03 p + (left operand) / 170; an accumulator gathers at most 64 + 2 of them (< 68 p, the layer holds 170 p)
// and is normalised after every addition; the sum of the 8 accumulators (< 544 p, top limb < 2^31) enters one product by W(1) as the
// LEFT operand, whose limbs may reach 3.28e9 (field29_dev.h), and leaves below 4.3 p < 2^256.
#include "ctx.h"
#include "msm.h"
#include "poly.h"
#include "field29_dev.h"
#include "kzg_multi_plan.h"
#include "kzg_scratch.h"
#include <cstring>
#include <string>
#include <vector>

namespace plk {

using host::KM_MAX_POLYS; using host::KM_MAX_OPEN; using host::KM_MAX_POINTS; using host::KM_TILE; using host::KM_THREADS; using host::KM_EPT;
using host::KM_LOG_THREADS; using host::KM_C_POW; using host::KM_C_LANE; using host::KM_C_TILE; using host::KM_C_CHUNK; using host::KM_CONSTS;
static_assert(KM_TILE == POLY_SCAN_BLOCK && KM_TILE == KM_THREADS * KM_EPT && KM_THREADS == (1u << KM_LOG_THREADS), "the scan engine's tile");

struct KmArgs {
    const Fr *f[KM_MAX_POLYS];
    uint8_t nz[KM_MAX_POLYS];           // bit j: coef[i][j] is not zero
    uint32_t count, n, npoints, ntiles;
    const Fr *coef;                     // count x KM_MAX_POINTS, W
    const Fr *cst;                      // KM_MAX_POINTS x KM_CONSTS, W (km_point_constants)
    Fr *tilev;                          // npoints x ntiles: the tiles' Horner values, after k_km_carry what stands above each tile
    Fr *out;
};

__device__ __forceinline__ FrW9 km_ldw(const Fr *p) { return unpack<FrW>(load_fp(p)); }

// row[tid] <- sum_{u >= tid} row[u] * P^(u - tid) over the 256 lanes, canonical in and out; step[s] = W(P^(2^s)).  The caller has
// synchronised after writing the row; the row is complete for every lane on return.
__device__ __forceinline__ void km_scan_row(Fr *row, const Fr *step, uint32_t tid) {
    FrW9 incl = unpack<FrW>(row[tid]);
#pragma unroll 1
    for (uint32_t s = 0; s < KM_LOG_THREADS; s++) {
        const uint32_t off = 1u << s;
        const bool have = tid + off < KM_THREADS;
        FrW9 o = w_zero<FrW>();
        if (have) o = unpack<FrW>(row[tid + off]);
        __syncthreads();
        if (have) { incl = reduce_small(addn(mulw(o, km_ldw(step + s)), incl)); row[tid] = pack<FrParams>(incl); }
        __syncthreads();
    }
}

template <int NP, bool PASS_B>
__global__ void __launch_bounds__(KM_THREADS) k_km_tiles(KmArgs a) {
    __shared__ __attribute__((aligned(16))) Fr sh[NP * KM_THREADS];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, base = tile * KM_TILE + tid * KM_EPT;
    FrW9 acc[NP], t[NP];
    static_for<NP>([&](auto J) {
        constexpr int j = decltype(J)::value;
        acc[j] = w_zero<FrW>();
        t[j] = km_ldw(a.cst + j * KM_CONSTS + KM_C_POW + 1);
    });
    // the walk: acc_j = H_j[l] restricted to this lane's coefficients.  PASS_B: what stands above l inside the lane, summed over the
    // points, goes to out[l]; the store follows the loads of position l, so `out` may be one of the polynomials (the second quotient of
    // an opening is written over h: only the lane that owns l reads or writes position l in this kernel).
    if constexpr (NP == 1) {
        // ONE POINT (every second quotient): the lane first forms G[l] for its 8 positions, polynomial by polynomial — its 8 loads of a
        // polynomial are 256 consecutive bytes, two cache lines used whole, where the walk below touches a quarter of a line per load —
        // and then walks.  8 x 9 accumulating words instead of 9; the stores still follow every load of the lane's positions.
        FrW9 g[KM_EPT];
        static_for<KM_EPT>([&](auto E) { g[decltype(E)::value] = w_zero<FrW>(); });
#pragma unroll 1
        for (uint32_t i = 0; i < a.count; i++) {
            if (!a.nz[i]) continue;
            const FrW9 c = km_ldw(a.coef + i * KM_MAX_POINTS);
            const Fr *f = a.f[i] + base;
            static_for<KM_EPT>([&](auto E) {
                constexpr int e = decltype(E)::value;
                if (base + e < a.n) g[e] = addn(g[e], mulw(km_ldw(f + e), c));
            });
        }
        static_for<KM_EPT>([&](auto E) {
            constexpr int e = (int)KM_EPT - 1 - decltype(E)::value;
            if (PASS_B && base + e < a.n) store_fp(a.out + base + e, pack<FrParams>(mulw(acc[0], w_one<FrW>())));
            acc[0] = e == (int)KM_EPT - 1 ? g[e] : addn(mulw(acc[0], t[0]), g[e]);
        });
    } else {
#pragma unroll 1
        for (int e = (int)KM_EPT - 1; e >= 0; e--) {
            const uint32_t l = base + (uint32_t)e;
            FrW9 above = acc[0];
            if (PASS_B) static_for<NP - 1>([&](auto J) { above = addn(above, acc[decltype(J)::value + 1]); });
            if (e != (int)KM_EPT - 1) static_for<NP>([&](auto J) { constexpr int j = decltype(J)::value; acc[j] = mulw(acc[j], t[j]); });
            if (l < a.n) {
#pragma unroll 1
                for (uint32_t i = 0; i < a.count; i++) {
                    const uint32_t m = a.nz[i];
                    if (!m) continue;
                    const FrW9 x = km_ldw(a.f[i] + l);
                    static_for<NP>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        if ((m >> j) & 1) acc[j] = addn(acc[j], mulw(x, km_ldw(a.coef + i * KM_MAX_POINTS + j)));
                    });
                }
                if (PASS_B) store_fp(a.out + l, pack<FrParams>(mulw(above, w_one<FrW>())));
            }
        }
    }
    // the lanes' Horner values, canonical; the value above the tile enters at the last lane, one lane further up (t^8)
    static_for<NP>([&](auto J) {
        constexpr int j = decltype(J)::value;
        FrW9 v = acc[j];
        if (PASS_B && tid == KM_THREADS - 1 && (uint32_t)j < a.npoints)
            v = addn(v, mulw(km_ldw(a.tilev + (size_t)j * a.ntiles + tile), km_ldw(a.cst + j * KM_CONSTS + KM_C_LANE)));
        sh[j * KM_THREADS + tid] = pack<FrParams>(csub_p(mulw(v, w_one<FrW>())));
    });
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < a.npoints; j++) km_scan_row(sh + j * KM_THREADS, a.cst + j * KM_CONSTS + KM_C_LANE, tid);
    if (!PASS_B) {
        if (tid < a.npoints) store_fp(a.tilev + (size_t)tid * a.ntiles + tile, sh[tid * KM_THREADS]);
        return;
    }
#pragma unroll 1
    for (uint32_t e = 0; e < KM_EPT; e++) {
        const uint32_t l = base + e;
        if (l >= a.n) break;
        FrW9 s = km_ldw(a.out + l);
#pragma unroll 1
        for (uint32_t j = 0; j < a.npoints; j++) {
            const FrW9 up = tid + 1 < KM_THREADS ? unpack<FrW>(sh[j * KM_THREADS + tid + 1]) : km_ldw(a.tilev + (size_t)j * a.ntiles + tile);
            s = addn(s, mulw(up, km_ldw(a.cst + j * KM_CONSTS + KM_C_POW + (KM_EPT - 1 - e))));
        }
        store_fp(a.out + l, pack<FrParams>(reduce_small(s)));
    }
}

// V[q] <- sum_{q' > q} V[q'] T^(q' - q - 1) for the point blockIdx.x, in place: each lane walks `per` consecutive tiles twice (its own
// Horner value, then, from what the scan says stands above its chunk, the value above each of its tiles)
__global__ void __launch_bounds__(KM_THREADS) k_km_carry(Fr *tilev, const Fr *cst, uint32_t ntiles, uint32_t per) {
    __shared__ __attribute__((aligned(16))) Fr sh[KM_THREADS];
    const uint32_t tid = threadIdx.x;
    Fr *V = tilev + (size_t)blockIdx.x * ntiles;
    const Fr *c = cst + blockIdx.x * KM_CONSTS;
    const uint32_t lo = tid * per < ntiles ? tid * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    const FrW9 T = km_ldw(c + KM_C_TILE);
    FrW9 acc = w_zero<FrW>();
    for (uint32_t q = hi; q-- > lo;) acc = addn(mulw(acc, T), km_ldw(V + q));
    sh[tid] = pack<FrParams>(reduce_small(acc));
    __syncthreads();
    km_scan_row(sh, c + KM_C_CHUNK, tid);
    acc = w_zero<FrW>();
    if (tid + 1 < KM_THREADS) acc = unpack<FrW>(sh[tid + 1]);
    for (uint32_t q = hi; q-- > lo;) {
        const FrW9 v = km_ldw(V + q);
        store_fp(V + q, pack<FrParams>(reduce_small(acc)));
        acc = addn(mulw(acc, T), v);
    }
}

namespace {
using namespace host;

inline Fr km_dev(const HFr &h) { Fr f; memcpy(f.l, h.l, 32); return f; }
inline HFr km_host(const plk_fr *p) { HFr h; memcpy(h.l, p->l, 32); return h; }
inline bool km_fr_ok(const plk_fr *p) { return !HFr::geq_p(p->l); }

// device scratch of one quotient, in elements: the constants, the matrix, one value per tile and point
inline size_t km_scratch_elems(uint64_t n, uint32_t npoints) { return (size_t)KM_MAX_POINTS * KM_CONSTS + (size_t)KM_MAX_POLYS * KM_MAX_POINTS + (size_t)npoints * km_tiles(n); }

template <bool PASS_B> void km_launch_tiles(uint32_t npoints, const KmArgs &a, hipStream_t st) {
    const dim3 grid(a.ntiles), block(KM_THREADS);
    if (npoints == 1) hipLaunchKernelGGL((k_km_tiles<1, PASS_B>), grid, block, 0, st, a);
    else if (npoints == 2) hipLaunchKernelGGL((k_km_tiles<2, PASS_B>), grid, block, 0, st, a);
    else if (npoints <= 4) hipLaunchKernelGGL((k_km_tiles<4, PASS_B>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_km_tiles<8, PASS_B>), grid, block, 0, st, a);
}

// out <- sum_j D_{t_j}[sum_i coef[i * npoints + j] f_i] on st; scratch: km_scratch_elems(n, npoints) elements.  `stage` is what the copies
// read: the caller keeps it until the stream has been waited for.  out may be one of the polynomials (k_km_tiles).
int32_t quotient_multi(const Fr *const *f, uint32_t count, uint64_t n, const HFr *points, uint32_t npoints, const HFr *coef, Fr *out, Fr *scratch,
                       std::vector<Fr> &stage, hipStream_t st) {
    KmArgs a{};
    a.count = count; a.n = (uint32_t)n; a.npoints = npoints; a.ntiles = km_tiles(n);
    const size_t head = (size_t)KM_MAX_POINTS * KM_CONSTS + (size_t)KM_MAX_POLYS * KM_MAX_POINTS;
    stage.assign(head, Fr::zero());
    HFr c[KM_CONSTS];
    for (uint32_t j = 0; j < KM_MAX_POINTS; j++) {                 // (a kernel instantiated for more points than the call has reads zero constants)
        km_point_constants(j < npoints ? points[j] : HFr::zero(), a.ntiles, c);
        for (uint32_t k = 0; k < KM_CONSTS; k++) stage[j * KM_CONSTS + k] = km_dev(c[k]);
    }
    for (uint32_t i = 0; i < count; i++) {
        a.f[i] = f[i];
        for (uint32_t j = 0; j < npoints; j++) {
            const HFr &v = coef[i * npoints + j];
            if (v.is_zero()) continue;
            a.nz[i] |= (uint8_t)(1u << j);
            stage[(size_t)KM_MAX_POINTS * KM_CONSTS + i * KM_MAX_POINTS + j] = km_dev(km_to_w(v));
        }
    }
    PLK_HIP(hipMemcpyAsync(scratch, stage.data(), head * sizeof(Fr), hipMemcpyHostToDevice, st));
    a.cst = scratch; a.coef = scratch + (size_t)KM_MAX_POINTS * KM_CONSTS; a.tilev = scratch + head; a.out = out;
    km_launch_tiles<false>(npoints, a, st);
    hipLaunchKernelGGL(k_km_carry, dim3(npoints), dim3(KM_THREADS), 0, st, a.tilev, a.cst, a.ntiles, km_chunk(a.ntiles));
    km_launch_tiles<true>(npoints, a, st);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

}  // namespace
int32_t km_common(const char *who, plk_ctx *ctx, const void *const *polys, uint32_t count, uint32_t max_count, uint64_t n, uint32_t npoints) {   // (kzg_scratch.h)
    if (!ctx || !polys || count == 0 || count > max_count || npoints == 0 || npoints > KM_MAX_POINTS || n == 0) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    for (uint32_t i = 0; i < count; i++) {
        if (!polys[i]) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
        if ((uintptr_t)polys[i] & 15u) { set_error(std::string(who) + ": device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    }
    if (n > (1ull << MAX_LOG_N)) { set_error(std::string(who) + ": more than 2^28 coefficients"); return PLK_ERR_SIZE; }
    if (ctx->combine) { set_error(std::string(who) + ": single-GPU only (this context holds one shard of a key, plk_set_commit_shard)"); return PLK_ERR_ARG; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error(std::string(who) + ": a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    return PLK_OK;
}
namespace {

int32_t open_multi(plk_ctx *ctx, const Fr *const *f, uint32_t count, uint64_t n, const HFr *points, uint32_t npoints, const uint32_t *sets, const HFr &gamma,
                   plk_kzg_challenge_fn challenge, void *user, plk_fr *evals, plk_fr *u_out, plk_g1_affine *proof, hipStream_t st) {
    const char *who = "plk_kzg_open_multi_dev";
    if (!ctx->srs().pts || n > ctx->srs().n) { set_error("plk_kzg_open_dev: no key resident, or the key is shorter than the polynomials"); return PLK_ERR_SRS; }
    HFr w[KM_MAX_OPEN * KM_MAX_POINTS], mat[(KM_MAX_OPEN + 1) * KM_MAX_POINTS];
    km_weights(points, npoints, sets, count, w);
    km_matrix(w, gamma, count, npoints, mat);
    // scratch: [ power tables of the points | evaluations | the quotients' constants, matrix and tile values | h ]
    const size_t tab_elems = (size_t)KM_MAX_POINTS * 2 * POW_TAB, res_elems = (size_t)KM_MAX_OPEN * KM_MAX_POINTS;
    KzgScratch ws(ctx, st);
    PLK_TRY(ws.reserve((tab_elems + res_elems + km_scratch_elems(n, npoints) + n) * sizeof(Fr)));
    Fr *tab = ctx->kzg_ws.as<Fr>(), *res = tab + tab_elems, *qs = res + res_elems, *h = qs + km_scratch_elems(n, npoints);
    StageTimer<6> ev;
    PLK_TRY(ev.start(ctx));
    PLK_TRY(ev.mark(0, st));
    // 1. y_ij = f_i(t_j) for j in S_i, twelve pairs per launch
    PowTable pt[KM_MAX_POINTS];
    for (uint32_t g = 0; g < npoints; g += 4) {
        Fr bases[4]; Fr *bufs[4];
        for (uint32_t k = 0; k < 4; k++) { bases[k] = km_dev(g + k < npoints ? points[g + k] : HFr::zero()); bufs[k] = tab + (size_t)(g + k) * 2 * POW_TAB; }
        PLK_TRY(fill_pow_tables4_into(ctx, bases, bufs, pt + g, st));
    }
    uint32_t pair_i[KM_MAX_OPEN * KM_MAX_POINTS], pair_j[KM_MAX_OPEN * KM_MAX_POINTS], pairs = 0;
    for (uint32_t i = 0; i < count; i++)
        for (uint32_t j = 0; j < npoints; j++) if ((sets[i] >> j) & 1) { pair_i[pairs] = i; pair_j[pairs] = j; pairs++; }
    for (uint32_t first = 0; first < pairs; first += EVAL_MAX) {
        EvalArgs ea{};
        ea.count = pairs - first < EVAL_MAX ? pairs - first : EVAL_MAX;
        for (uint32_t k = 0; k < ea.count; k++) { ea.poly[k] = f[pair_i[first + k]]; ea.len[k] = (uint32_t)n; ea.pt[k] = pt[pair_j[first + k]]; }
        PLK_TRY(eval_batch(ctx, ea, res + first, st));
    }
    std::vector<HFr> ys(pairs);
    PLK_HIP(hipMemcpyAsync(ys.data(), res, pairs * sizeof(Fr), hipMemcpyDeviceToHost, st));
    PLK_TRY(ev.mark(1, st));
    // 2. h = sum_j D_{t_j}[sum_i gamma^i w_ij f_i] and W = commit(h)
    std::vector<Fr> stage1, stage2;
    PLK_TRY(quotient_multi(f, count, n, points, npoints, mat, h, qs, stage1, st));
    PLK_TRY(ev.mark(2, st));
    PLK_TRY(msm_commit(ctx, ctx->srs(), h, n, 0, &proof[0], st));   // waits: the evaluations have arrived as well
    PLK_TRY(ev.mark(3, st));
    for (uint32_t k = 0; k < count * npoints; k++) memset(evals[k].l, 0, 32);
    for (uint32_t k = 0; k < pairs; k++) memcpy(evals[pair_i[k] * npoints + pair_j[k]].l, ys[k].l, 32);
    // 3. the caller's challenge, once
    plk_fr u_raw;
    memset(&u_raw, 0, sizeof u_raw);
    const int32_t rc = challenge(user, &proof[0], &u_raw);
    if (rc != 0) { set_error(std::string(who) + ": the challenge callback returned " + std::to_string(rc)); return PLK_ERR_IO; }
    if (!km_fr_ok(&u_raw)) { set_error(std::string(who) + ": the challenge callback gave a scalar that is not below r"); return PLK_ERR_ARG; }
    const HFr u = km_host(&u_raw);
    *u_out = u_raw;
    // 4. W' = commit(D_u[sum_i c_i f_i - Z_T(u) h]): the same operator, one point, the polynomials and h; written over h
    HFr c[KM_MAX_OPEN + 1], z_t;
    km_c(points, npoints, sets, count, gamma, u, c, &z_t);
    c[count] = -z_t;
    const Fr *f2[KM_MAX_OPEN + 1];
    for (uint32_t i = 0; i < count; i++) f2[i] = f[i];
    f2[count] = h;
    PLK_TRY(ev.mark(4, st));
    PLK_TRY(quotient_multi(f2, count + 1, n, &u, 1, c, h, qs, stage2, st));
    PLK_TRY(msm_commit(ctx, ctx->srs(), h, n, 0, &proof[1], st));
    PLK_TRY(ev.mark(5, st));
    if (ev.on) {
        PLK_HIP(hipEventSynchronize(ev.e[5]));
        for (int k = 0; k < 3; k++) PLK_TRY(ev.elapsed(k, k + 1, &ctx->km_ms[k]));
        PLK_TRY(ev.elapsed(4, 5, &ctx->km_ms[3]));
        ctx->km_ms_valid = true;
    }
    return PLK_OK;
}

}  // namespace
}  // namespace plk

using namespace plk;
using namespace plk::host;

extern "C" int32_t plk_poly_quotient_multi_dev(plk_ctx *ctx, const void *const *polys_dev, uint32_t count, uint64_t n, const plk_fr *points, uint32_t npoints,
                                               const plk_fr *coef, void *out_dev, void *stream) {
    const char *who = "plk_poly_quotient_multi_dev";
    if (!points || !coef || !out_dev) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    PLK_TRY(km_common(who, ctx, polys_dev, count, KM_MAX_POLYS, n, npoints));
    if ((uintptr_t)out_dev & 15u) { set_error(std::string(who) + ": device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    const uintptr_t span = (uintptr_t)n * sizeof(Fr), o = (uintptr_t)out_dev;
    for (uint32_t i = 0; i < count; i++) {
        const uintptr_t p = (uintptr_t)polys_dev[i];
        if (o < p + span && p < o + span) { set_error(std::string(who) + ": the output overlaps polynomial " + std::to_string(i)); return PLK_ERR_ARG; }
    }
    HFr pts[KM_MAX_POINTS];
    std::vector<HFr> cf((size_t)count * npoints);
    for (uint32_t j = 0; j < npoints; j++) {
        if (!km_fr_ok(points + j)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
        pts[j] = km_host(points + j);
    }
    for (size_t k = 0; k < cf.size(); k++) {
        if (!km_fr_ok(coef + k)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
        cf[k] = km_host(coef + k);
    }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    try {
        KzgScratch ws(ctx, st);
        PLK_TRY(ws.reserve(km_scratch_elems(n, npoints) * sizeof(Fr)));
        std::vector<Fr> stage;
        PLK_TRY(quotient_multi(reinterpret_cast<const Fr *const *>(polys_dev), count, n, pts, npoints, cf.data(), static_cast<Fr *>(out_dev), ctx->kzg_ws.as<Fr>(), stage, st));
        PLK_HIP(hipStreamSynchronize(st));
        return PLK_OK;
    } catch (const std::exception &e) { set_error(std::string(who) + ": " + e.what()); return PLK_ERR_HIP; }
}

extern "C" int32_t plk_kzg_open_multi_dev(plk_ctx *ctx, const void *const *polys_dev, uint32_t count, uint64_t n, const plk_fr *points, uint32_t npoints,
                                          const uint32_t *sets, const plk_fr *gamma, plk_kzg_challenge_fn challenge, void *user, plk_fr *evals, plk_fr *u_out,
                                          plk_g1_affine proof[2], void *stream) {
    const char *who = "plk_kzg_open_multi_dev";
    if (ctx) ctx->km_ms_valid = false;
    if (!points || !sets || !gamma || !challenge || !evals || !u_out || !proof) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    PLK_TRY(km_common(who, ctx, polys_dev, count, KM_MAX_OPEN, n, npoints));
    HFr pts[KM_MAX_POINTS];
    for (uint32_t j = 0; j < npoints; j++) {
        if (!km_fr_ok(points + j)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
        pts[j] = km_host(points + j);
    }
    if (!km_fr_ok(gamma)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
    const int verdict = km_check_sets(pts, npoints, sets, count);
    if (verdict != KM_SETS_OK) { set_error(std::string(who) + ": " + km_sets_words(verdict)); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    try {
        return open_multi(ctx, reinterpret_cast<const Fr *const *>(polys_dev), count, n, pts, npoints, sets, km_host(gamma), challenge, user, evals, u_out, proof, st);
    } catch (const std::exception &e) { set_error(std::string(who) + ": " + e.what()); return PLK_ERR_HIP; }
}

extern "C" int32_t plk_kzg_open_multi_last_ms(plk_ctx *ctx, float out_ms[4]) {
    if (!ctx || !out_ms) { set_error("plk_kzg_open_multi_last_ms: bad argument"); return PLK_ERR_ARG; }
    if (!ctx->km_ms_valid) { set_error("plk_kzg_open_multi_last_ms: no timed plk_kzg_open_multi_dev on this context (plk_set_kernel_timing)"); return PLK_ERR_ARG; }
    for (int k = 0; k < 4; k++) out_ms[k] = ctx->km_ms[k];
    return PLK_OK;
}

extern "C" int32_t plk_kzg_verify_multi(const plk_g1_affine *commitments, uint32_t count, const plk_fr *points, uint32_t npoints, const uint32_t *sets,
                                        const plk_fr *evals, const plk_fr *gamma, const plk_fr *u, const plk_g1_affine proof[2], const uint8_t g2[256], int32_t *valid) {
    const char *who = "plk_kzg_verify_multi";
    if (valid) *valid = 0;
    if (!commitments || !points || !sets || !evals || !gamma || !u || !proof || !g2 || !valid || count == 0 || count > KM_MAX_OPEN || npoints == 0 || npoints > KM_MAX_POINTS) {
        set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    auto point_ok = [](const plk_g1_affine *p, HAffine *o) {
        memcpy(o, p, 64);
        return o->is_inf() || (!HFq::geq_p(p->x) && !HFq::geq_p(p->y) && on_curve(*o));
    };
    HAffine W[2];
    for (int k = 0; k < 2; k++)
        if (!point_ok(proof + k, &W[k])) { set_error(std::string(who) + ": the proof is not a point of the curve"); return PLK_ERR_ARG; }
    HFr pts[KM_MAX_POINTS];
    for (uint32_t j = 0; j < npoints; j++) {
        if (!km_fr_ok(points + j)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
        pts[j] = km_host(points + j);
    }
    if (!km_fr_ok(gamma) || !km_fr_ok(u)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
    const int verdict = km_check_sets(pts, npoints, sets, count);
    if (verdict != KM_SETS_OK) { set_error(std::string(who) + ": " + km_sets_words(verdict)); return PLK_ERR_ARG; }
    const HFr g = km_host(gamma), uu = km_host(u);
    HFr w[KM_MAX_OPEN * KM_MAX_POINTS], c[KM_MAX_OPEN], z_t, R = HFr::zero();
    km_weights(pts, npoints, sets, count, w);
    km_c(pts, npoints, sets, count, g, uu, c, &z_t);
    // F = sum_i c_i C_i - (sum_i c_i r_i(u)) G - Z_T(u) W
    HJac F = HJac::inf();
    uint64_t k[4];
    for (uint32_t i = 0; i < count; i++) {
        HAffine ci;
        if (!point_ok(commitments + i, &ci)) { set_error(std::string(who) + ": commitment " + std::to_string(i) + " is not a point of the curve"); return PLK_ERR_ARG; }
        HFr y[KM_MAX_POINTS];
        for (uint32_t j = 0; j < npoints; j++) {
            y[j] = HFr::zero();
            if (!((sets[i] >> j) & 1)) continue;
            if (!km_fr_ok(evals + i * npoints + j)) { set_error(std::string(who) + ": a scalar is not below r"); return PLK_ERR_ARG; }
            y[j] = km_host(evals + i * npoints + j);
        }
        R = R + c[i] * km_r_at(pts, npoints, sets[i], w + i * npoints, y, uu);
        c[i].to_canonical(k);
        F = jac_add(F, jac_mul(jac_from_affine(ci), k));
    }
    HAffine gen; gen.x = HFq::one(); gen.y = HFq::one() + HFq::one();
    (-R).to_canonical(k);
    F = jac_add(F, jac_mul(jac_from_affine(gen), k));
    (-z_t).to_canonical(k);
    F = jac_add(F, jac_mul(jac_from_affine(W[0]), k));
    uu.to_canonical(k);
    const HJac A = jac_add(F, jac_mul(jac_from_affine(W[1]), k));
    const HAffine a = jac_to_affine(A), b = jac_to_affine(jac_neg(jac_from_affine(W[1])));
    plk_g1_affine pa, pb;
    memcpy(&pa, &a, 64); memcpy(&pb, &b, 64);
    return plk_pairing_check(&pa, g2, &pb, g2 + 128, valid);
}
