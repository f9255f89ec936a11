// Inverse NTT over G1 — `plonkit dump-lagrange`:
//   Crs::<Bn256, CrsForLagrangeForm>::from_powers(&mono, n.next_power_of_two(), &Worker)
//   (src/plonk.rs:179-185; driven from src/bin/main.rs:360-381).
// in[j] = tau^j * G  ->  out[i] = L_i(tau) * G, the Lagrange-basis SRS of the size-N domain.
// Radix-2 DIT over group elements: a butterfly is (A, B) -> (A + w*B, A - w*B) where w*B is a full 254-bit scalar
// multiplication, so the kernel is bound by v_mad_u64_u32 issue and HBM traffic (144 B per point per stage) is
// negligible.  One lane per butterfly, XYZZ coordinates on the 9 x 29-bit layer between stages, a single Fermat
// inversion per point at the end; 1/N rides on the last stage (N/2 extra scalar multiplications, not N).
//
// Scalar multiplication on a SIMT machine: with double-and-add (or any sparse recoding) some lane of the wave has a
// non-zero digit at nearly every bit, so the whole wave pays one addition per bit.  Fixed signed 3-bit windows make
// all lanes add at the same positions; the window table {1,2,3,4}*B of every lane lives in LDS, limb-major
// (conflict-free).  Round 1: 255 doublings + 85 additions (~3500 field products).  Round 4: the GLV endomorphism halves
// the doubling chain — 129 doublings + 86 additions + 43 products by beta (~2400), see g1_mul_scalar / glv_dev.h.  Round 6: the window table made
// effectively affine on an isomorphic curve (eight points, 4-bit windows, mixed additions): ~1960, see g1_mul_scalar_iso8.
#include "ctx.h"
#include "ec_dev.h"
#include "ec29_dev.h"
#include "glv_dev.h"
#include "g1_mul_dev.h"
#include "ntt.h"
#include "kzg_all_plan.h"
#include <type_traits>

namespace plk {

__device__ __forceinline__ uint32_t brev32(uint32_t x, uint32_t bits) { return bits ? (__brev(x) >> (32 - bits)) : 0; }


// pts[bitrev(i)] = in[i]   (in: affine, external form; pts: XYZZ on the 29-bit layer).  The factor 1/N is applied by the LAST stage
// (g1ntt_stage, SCALE): there half of the points are multiplied by a twiddle anyway, which takes 1/N along for nothing, so the
// scaling costs N/2 scalar multiplications instead of the N of a pass of its own (one stage's worth of the transform's 22).
// `count` arrays of 2^log_n points back to back, each permuted inside itself (count << log_n <= 2^26: the flattened index fits 32 bits)
__global__ void __launch_bounds__(256) g1ntt_load(XyzzW *pts, const G1Affine *in, uint32_t log_n, uint32_t count) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (count << log_n)) return;
    const G1Affine a = load_affine(in + i);
    XyzzW p = xyzzw_identity();
    if (!is_inf(a)) {
        p.x = csub_p(w_from_s(unpack<FqW>(a.x))); p.y = csub_p(w_from_s(unpack<FqW>(a.y)));
        p.zz = w_one<FqW>(); p.zzz = w_one<FqW>();
    }
    const uint32_t k = i & ((1u << log_n) - 1);
    store_xyzzw(pts + (i - k) + brev32(k, log_n), p);
}

// the same permutation of points that are XYZZ already, where they lie: the lane of the lower index of a pair swaps it.  `count` arrays whose
// first points lie `stride` points apart (fk_batch_point), the first 2^log_n of each
__global__ void __launch_bounds__(256) g1ntt_bitrev(XyzzW *pts, uint32_t log_n, uint32_t count, uint32_t stride) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (count << log_n)) return;
    const uint32_t i = g & ((1u << log_n) - 1), r = brev32(i, log_n);
    if (i >= r) return;
    pts += fk_batch_point(log_n, stride, g) - i;
    const XyzzW a = load_xyzzw(pts + i), b = load_xyzzw(pts + r);
    store_xyzzw(pts + i, b);
    store_xyzzw(pts + r, a);
}

// one DIT stage with half-size h = 2^s; SCALE (the last stage): both outputs times n_inv (Montgomery form) — (A n_inv) +- (w n_inv) B
// tw: the powers of omega^-1 (inverse transform) or of omega (forward: never with SCALE)
// One launch covers `count` transforms whose first points lie `stride` points apart; the transform is the SLOW index of the launch
// (fk_batch_butterfly, kzg_all_plan.h), so transforms of fewer than 256 butterflies share a workgroup, of fewer than 64 a wave, and a
// single transform is a batch of one.  count << (log_n - 1) <= 2^25.
template <bool SCALE, int ISO>
__global__ void __launch_bounds__(G1NTT_THREADS, 1) g1ntt_stage(XyzzW *pts, uint32_t log_n, uint32_t s, PowTable tw, Fr n_inv, uint32_t count, uint32_t stride) {
    extern __shared__ uint32_t g1tab[];
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (count << (log_n - 1))) return;
    const FkButterfly bf = fk_batch_butterfly(log_n, g);
    pts += (size_t)bf.poly * stride;
    // butterfly j of the stage: group jh, position jl inside the half (twiddle exponent).  jl = 0 needs no multiplication; in the early
    // stages (h < 64) consecutive lanes would all differ in jl and every wave would pay for the one lane in h that has it.  There the
    // position is the SLOW index of the launch: whole waves (workgroups) share jl, and those with jl = 0 — half of stage 1, a quarter of
    // stage 2, .. — only add.  (The accesses become strided; memory traffic is nothing in this kernel.)  fk_stage_pair has the two forms.
    const FkPair pr = fk_stage_pair(log_n, s, bf.j);
    const uint32_t jl = pr.jl, i0 = pr.i0, i1 = pr.i1;
    XyzzW a = load_xyzzw(pts + i0), b = load_xyzzw(pts + i1);
    if (jl || SCALE) {
        Fr w = n_inv;
        if (jl) {
            // omega_N^-+(jl * N / 2h)
            uint32_t e = (jl << (log_n - s - 1)) << (MAX_LOG_N - log_n);
            w = mul(load_fp(tw.lo + (e & (POW_TAB - 1))), load_fp(tw.hi + (e >> POW_SPLIT)));
            if (SCALE) w = mul(w, n_inv);
        }
        auto mul = [&](const XyzzW &pt, const Fr &kk) __attribute__((always_inline)) {
            if constexpr (ISO == 2) return g1_mul_scalar_iso8(pt, kk, g1tab);
            else if constexpr (ISO == 1) return g1_mul_scalar_iso(pt, kk, g1tab);
            else return g1_mul_scalar(pt, kk, g1tab);
        };
        b = mul(b, to_canonical(w));
        if (SCALE) a = mul(a, to_canonical(n_inv));
    }
    XyzzW lo = a, nb = b;
    nb.y = sub6(w_zero<FqW>(), b.y);
    g1_add_call(&lo, &b);
    g1_add_call(&a, &nb);
    store_xyzzw(pts + i0, lo);
    store_xyzzw(pts + i1, a);
}

// XYZZ -> affine with ONE field inversion per G1NTT_NORM_K points (Montgomery's trick on ZZZ; 1 / Z = ZZ / ZZZ, as srs_normalise_kernel does for the MSM table):
// a Fermat inversion per point was 4.3 ms of a 2^20-point transform.  A thread takes K consecutive points; the second walk reads them again (four products each)
// rather than keep K x 32 words alive.  Same canonical coordinates as before, bit for bit.
// out is dense; output point i < n = count << log_n is read at fk_batch_point(log_n, stride, i): the first 2^log_n of arrays `stride` points
// apart.  The groups of K need not line up with the arrays: the affine coordinates do not depend on what shares an inversion.
constexpr uint32_t G1NTT_NORM_K = 8;
__global__ void __launch_bounds__(256) g1ntt_to_affine(G1Affine *out, const XyzzW *pts, uint32_t n, uint32_t log_n, uint32_t stride) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lo = t * G1NTT_NORM_K, hi = lo + G1NTT_NORM_K < n ? lo + G1NTT_NORM_K : n;
    if (lo >= n) return;
    Fq prefix[G1NTT_NORM_K];
    Fq acc = Fq::one();
#pragma unroll
    for (uint32_t j = 0; j < G1NTT_NORM_K; j++) {
        if (lo + j < hi) {
            const XyzzW w = load_xyzzw(pts + fk_batch_point(log_n, stride, lo + j));
            if (!is_inf(w)) acc = mul(acc, pack<FqParams>(s_from_w(w.zzz)));
        }
        prefix[j] = acc;
    }
    Fq inv_acc = inv(acc);
#pragma unroll
    for (uint32_t jj = 0; jj < G1NTT_NORM_K; jj++) {
        const uint32_t j = G1NTT_NORM_K - 1 - jj;
        if (lo + j >= hi) continue;
        const G1Xyzz q = xyzzw_export(load_xyzzw(pts + fk_batch_point(log_n, stride, lo + j)));  // back to the external form (canonical, R = 2^256); the identity is all zero
        G1Affine a; a.x = Fq::zero(); a.y = Fq::zero();
        if (!is_inf(q)) {
            const Fq zi = j ? mul(inv_acc, prefix[j - 1]) : inv_acc;  // 1 / ZZZ_j
            inv_acc = mul(inv_acc, q.zzz);
            const Fq iz = mul(q.zz, zi), izz = mul(iz, iz);       // 1 / Z, 1 / ZZ
            a.x = mul(q.x, izz);
            a.y = mul(q.y, zi);
        }
        store_fp(&out[lo + j].x, a.x);
        store_fp(&out[lo + j].y, a.y);
    }
}

// dynamic LDS of the six stage instantiations, once per process
static int32_t g1ntt_stage_attrs() {
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(g1ntt_stage<false, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS));
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(g1ntt_stage<true, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS));
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(g1ntt_stage<false, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO));
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(g1ntt_stage<true, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO));
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(g1ntt_stage<false, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO8));
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(g1ntt_stage<true, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO8));
        attr_set = true;
    }
    return PLK_OK;
}

// The log_n stages over points already in bit-reversed order.  Inverse: omega^-1 and 1/N on the last stage.  Forward: omega, and the last stage is
// the non-scaling instantiation like the others (no multiplication by 1 goes through the SCALE path).
// `count` transforms `stride` points apart in every launch.
static int32_t g1ntt_stages(plk_ctx *ctx, XyzzW *pts, uint32_t count, uint32_t stride, uint32_t log_n, bool inverse, hipStream_t st) {
    PLK_TRY(g1ntt_stage_attrs());
    const uint32_t half = log_n ? count << (log_n - 1) : 0;       // butterflies of a launch
    const Fr n_inv = ctx->n_inv[log_n];                           // Montgomery form; 1 for log_n = 0 (no stage, nothing to scale)
    const PowTable tw = inverse ? ctx->tw_inv : ctx->tw_fwd;
    // PLK_G1NTT_ISO (A/B knob): 0 = the window table in XYZZ and full additions, as in rounds 4-5; 1 = four effectively affine entries, 3-bit windows; default 2 = eight, 4-bit windows
    // (the same chain in Jacobian coordinates — 4S + 3M doublings — was built, verified and measured 3 % SLOWER: profiles/r06b_g1ntt_jacobian.patch)
    static const int iso = [] { const char *e = getenv("PLK_G1NTT_ISO"); return e ? atoi(e) : 2; }();
    const dim3 sgrid((half + G1NTT_THREADS - 1) / G1NTT_THREADS);
    auto stage = [&](auto scale_tag, uint32_t s) {
        constexpr bool SC = decltype(scale_tag)::value;
        if (iso == 2) hipLaunchKernelGGL((g1ntt_stage<SC, 2>), sgrid, dim3(G1NTT_THREADS), G1NTT_LDS_ISO8, st, pts, log_n, s, tw, n_inv, count, stride);
        else if (iso == 1) hipLaunchKernelGGL((g1ntt_stage<SC, 1>), sgrid, dim3(G1NTT_THREADS), G1NTT_LDS_ISO, st, pts, log_n, s, tw, n_inv, count, stride);
        else hipLaunchKernelGGL((g1ntt_stage<SC, 0>), sgrid, dim3(G1NTT_THREADS), G1NTT_LDS, st, pts, log_n, s, tw, n_inv, count, stride);
    };
    for (uint32_t s = 0; s + 1 < log_n; s++) stage(std::false_type{}, s);
    if (log_n) { if (inverse) stage(std::true_type{}, log_n - 1); else stage(std::false_type{}, log_n - 1); }
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

// `count` arrays of 2^log_n points back to back, each transformed on its own
int32_t g1_ntt_dev(plk_ctx *ctx, const G1Affine *in, uint32_t count, uint32_t log_n, bool inverse, G1Affine *out, hipStream_t st, const char *who) {
    if (!fk_batch_points_ok(count, log_n)) { set_error(std::string(who) + ": size exceeds 2^26"); return PLK_ERR_SIZE; }
    PLK_TRY(ntt_init_tables(ctx));
    const uint32_t n = count << log_n;
    // the transform borrows the scratch of the first commitment slot: nothing may be in flight there
    if (ctx->msm_enq != ctx->msm_fin) { set_error(std::string(who) + ": a commitment enqueued with plk_msm_g1_enqueue_dev is still in flight (call plk_msm_g1_finish first)"); return PLK_ERR_ARG; }
    PLK_TRY(ctx->slot[0].c.reserve((size_t)n * sizeof(XyzzW)));
    XyzzW *pts = ctx->slot[0].c.as<XyzzW>();
    hipLaunchKernelGGL(g1ntt_load, dim3((n + 255) / 256), dim3(256), 0, st, pts, in, log_n, count);
    PLK_TRY(g1ntt_stages(ctx, pts, count, 1u << log_n, log_n, inverse, st));
    hipLaunchKernelGGL(g1ntt_to_affine, dim3(((n + G1NTT_NORM_K - 1) / G1NTT_NORM_K + 255) / 256), dim3(256), 0, st, out, (const XyzzW *)pts, n, log_n, 1u << log_n);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

int32_t g1_intt_dev(plk_ctx *ctx, const G1Affine *in, uint32_t log_n, G1Affine *out, hipStream_t st) { return g1_ntt_dev(ctx, in, 1, log_n, true, out, st, "g1_intt"); }

// The transform of 2^log_n XYZZ points where they lie (natural order in and out, any buffer of the caller's: no scratch, no refusal of its own
// beyond the size).  A chain of transforms (kzg_all.hip) stays on the 29-bit layer and pays for g1ntt_to_affine once.
// `count` transforms in every launch, over the first 2^log_n points of arrays `stride` >= 2^log_n points apart; count * stride <= 2^26.
int32_t g1_ntt_xyzzw_dev(plk_ctx *ctx, XyzzW *pts, uint32_t count, uint32_t stride, uint32_t log_n, bool inverse, hipStream_t st) {
    if (!fk_batch_points_ok(count, log_n) || stride < (1u << log_n) || (uint64_t)count * stride > ((uint64_t)1 << FK_BATCH_LOG_POINTS)) { set_error("g1_ntt: size exceeds 2^26"); return PLK_ERR_SIZE; }
    PLK_TRY(ntt_init_tables(ctx));
    const uint32_t n = count << log_n;
    hipLaunchKernelGGL(g1ntt_bitrev, dim3((n + 255) / 256), dim3(256), 0, st, pts, log_n, count, stride);
    return g1ntt_stages(ctx, pts, count, stride, log_n, inverse, st);
}
// out[b << log_n | i] = the affine form of pts[b * stride + i], b < count, i < 2^log_n
int32_t g1_xyzzw_to_affine_dev(const XyzzW *pts, uint32_t count, uint32_t stride, uint32_t log_n, G1Affine *out, hipStream_t st) {
    const uint32_t n = count << log_n;
    hipLaunchKernelGGL(g1ntt_to_affine, dim3(((n + G1NTT_NORM_K - 1) / G1NTT_NORM_K + 255) / 256), dim3(256), 0, st, out, pts, n, log_n, stride);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

}  // namespace plk

using namespace plk;

extern "C" int32_t plk_g1_intt(plk_ctx *ctx, const plk_g1_affine *in, uint32_t log_n, plk_g1_affine *out) {
    if (!ctx || !in || !out) { set_error("plk_g1_intt: bad argument"); return PLK_ERR_ARG; }
    if (log_n > 26) { set_error("g1_intt: size exceeds 2^26"); return PLK_ERR_SIZE; }
    PLK_HIP(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(plk_g1_affine) << log_n;
    PLK_TRY(ctx->stage.reserve(2 * bytes));
    G1Affine *d_in = ctx->stage.as<G1Affine>(), *d_out = d_in + ((size_t)1 << log_n);
    PLK_HIP(hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, ctx->stream));
    PLK_TRY(g1_intt_dev(ctx, d_in, log_n, d_out, ctx->stream));
    PLK_HIP(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PLK_HIP(hipStreamSynchronize(ctx->stream));
    return PLK_OK;
}

// the same transform applied to the first 2^log_n points of the resident SRS; result left on the device
extern "C" int32_t plk_g1_intt_srs_dev(plk_ctx *ctx, uint32_t log_n, void *out_dev, void *stream) {
    if (!ctx || !out_dev) { set_error("plk_g1_intt_srs_dev: bad argument"); return PLK_ERR_ARG; }
    if (!ctx->srs().pts || ctx->srs().n < ((uint64_t)1 << log_n)) { set_error("g1_intt: SRS too small"); return PLK_ERR_SRS; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    return g1_intt_dev(ctx, reinterpret_cast<const G1Affine *>(ctx->srs().pts), log_n, reinterpret_cast<G1Affine *>(out_dev), s);
}

// either direction, device to device: inverse != 0 is plk_g1_intt's transform, bit for bit; inverse == 0 is out[i] = sum_j omega^(i j) in[j]
extern "C" int32_t plk_g1_ntt_dev(plk_ctx *ctx, const void *in_dev, uint32_t log_n, int32_t inverse, void *out_dev, void *stream) {
    if (!ctx || !in_dev || !out_dev) { set_error("plk_g1_ntt_dev: bad argument"); return PLK_ERR_ARG; }
    if (((uintptr_t)in_dev | (uintptr_t)out_dev) & 15u) { set_error("plk_g1_ntt_dev: device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    return g1_ntt_dev(ctx, static_cast<const G1Affine *>(in_dev), 1, log_n, inverse != 0, static_cast<G1Affine *>(out_dev), s, "plk_g1_ntt_dev");
}

// the same transform over `count` arrays of 2^log_n points back to back, every stage of all of them in one launch
extern "C" int32_t plk_g1_ntt_batch_dev(plk_ctx *ctx, const void *in_dev, uint32_t count, uint32_t log_n, int32_t inverse, void *out_dev, void *stream) {
    if (!ctx || !in_dev || !out_dev) { set_error("plk_g1_ntt_batch_dev: bad argument"); return PLK_ERR_ARG; }
    if (count == 0) { set_error("plk_g1_ntt_batch_dev: count must be at least 1"); return PLK_ERR_ARG; }
    if (((uintptr_t)in_dev | (uintptr_t)out_dev) & 15u) { set_error("plk_g1_ntt_batch_dev: device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    return g1_ntt_dev(ctx, static_cast<const G1Affine *>(in_dev), count, log_n, inverse != 0, static_cast<G1Affine *>(out_dev), s, "plk_g1_ntt_batch_dev");
}
