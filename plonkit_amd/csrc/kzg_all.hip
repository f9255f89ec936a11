// KZG: the openings at ALL points of the domain in one pass (Feist-Khovratovich).  N calls of plk_kzg_open_dev cost N commitments; here the N
// quotient commitments h_k come out of one cyclic correlation of length 2N between the coefficients and the key, and the N proofs are DFT_N(h):
// three G1 transforms and 2N scalar multiplications.  The index maps, the sizes and the limits are kzg_all_plan.h's (its head has the
// mathematics); the transforms are g1ntt.hip's stage kernel in both directions, the multiplication is g1_mul_dev.h's.
// NO COUNTERPART IN THE REFERENCE: bellman's kate_commitment (reached from src/plonk.rs:4) opens at one point per call.
//
//   k_fk_arrange_t   t from the resident key (affine -> XYZZ on the 29-bit layer, identities elsewhere); forward G1 transform at 2N.  ONCE PER KEY
//                    and size: the result stays with the context (ctx->fk_key) until the key changes.
//   k_fk_arrange_c   c from the coefficients; the scalar NTT at 2N
//   k_fk_pointwise   u_m = c^_m * t^_m, one lane per point
//   inverse G1 transform at 2N (1 / 2N on its last stage), forward at N over the first N entries where they lie, g1ntt_to_affine once.
// A BATCH (plk_kzg_open_all_batch_dev) is `count` polynomials under the one key: every kernel above but k_fk_arrange_t runs over count x 2N
// entries with the polynomial as the slow index, t^ is read at m mod 2N, and every stage launch of g1ntt.hip covers all the transforms
// (stride 2N between them).  The single call is a batch of one.
#include "ctx.h"
#include "ntt.h"
#include "ec_dev.h"
#include "ec29_dev.h"
#include "glv_dev.h"
#include "g1_mul_dev.h"
#include "kzg_all_plan.h"
#include <string>

namespace plk {

int32_t g1_ntt_xyzzw_dev(plk_ctx *ctx, XyzzW *pts, uint32_t count, uint32_t stride, uint32_t log_n, bool inverse, hipStream_t st);     // g1ntt.hip
int32_t g1_xyzzw_to_affine_dev(const XyzzW *pts, uint32_t count, uint32_t stride, uint32_t log_n, G1Affine *out, hipStream_t st);        // g1ntt.hip

static_assert(sizeof(XyzzW) == FK_XYZZW_BYTES && sizeof(G1Affine) == FK_AFFINE_BYTES && sizeof(Fr) == FK_FR_BYTES, "kzg_all_plan.h sizes the buffers");
static_assert(FK_MAX_LOG_N + 1 <= 26, "the 2N-point transforms are within g1ntt's limit");

// c[b * 2N + m] for m < 2N from f[b * N ..], b < count
__global__ void __launch_bounds__(256) k_fk_arrange_c(Fr *c, const Fr *f, uint32_t log_n, uint32_t count) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (count << (log_n + 1))) return;
    const uint32_t b = g >> (log_n + 1), src = fk_c_source(log_n, g & ((2u << log_n) - 1));
    store_fp(c + g, src == FK_NONE ? Fr::zero() : load_fp(f + ((size_t)b << log_n) + src));
}

// t[m] for m < 2N; reads key points 0 .. N - 2 only
__global__ void __launch_bounds__(256) k_fk_arrange_t(XyzzW *t, const G1Affine *key, uint32_t log_n) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (2u << log_n)) return;
    const uint32_t src = fk_t_source(log_n, m);
    XyzzW p = xyzzw_identity();
    if (src != FK_NONE) {
        const G1Affine a = load_affine(key + src);
        if (!is_inf(a)) {
            p.x = csub_p(w_from_s(unpack<FqW>(a.x))); p.y = csub_p(w_from_s(unpack<FqW>(a.y)));
            p.zz = w_one<FqW>(); p.zzz = w_one<FqW>();
        }
    }
    store_xyzzw(t + m, p);
}

// u[m] = c_hat[m] * t_hat[m & mask] for m < count (mask = 2N - 1: the polynomials of a batch share the key's transform): g1ntt_stage's multiplication (eight effectively affine window points per lane in LDS, limb-major)
// without the butterfly.  A zero scalar or the identity gives the identity and takes no part in the multiplication.
__global__ void __launch_bounds__(G1NTT_THREADS, 1) k_fk_pointwise(XyzzW *u, const Fr *c_hat, const XyzzW *t_hat, uint32_t count, uint32_t mask) {
    extern __shared__ uint32_t g1tab[];
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= count) return;
    const Fr k = load_fp(c_hat + m);
    XyzzW p = load_xyzzw(t_hat + (m & mask));
    if (k.is_zero() || is_inf(p)) p = xyzzw_identity();
    else p = g1_mul_scalar_iso8(p, to_canonical(k), g1tab);
    store_xyzzw(u + m, p);
}

namespace {

// the scratch of a call: grows only, given back on the way out when the call grew it past FK_KEEP_BYTES (ctx->kzg_ws's rule)
struct FkWs {
    plk_ctx *ctx; hipStream_t st; bool grew = false;
    FkWs(plk_ctx *c, hipStream_t s) : ctx(c), st(s) {}
    int32_t reserve(size_t bytes) {
        if (bytes > ctx->fk_ws.cap) { grew = true; PLK_HIP(hipStreamSynchronize(st)); }
        return ctx->fk_ws.reserve(bytes);
    }
    ~FkWs() { if (grew && ctx->fk_ws.cap > FK_KEEP_BYTES) { (void)hipStreamSynchronize(st); ctx->fk_ws.release(); } }
};

// what every entry point of this file refuses, in this order: the size (of a polynomial, then of the batch), a sharded key, a commitment in flight, a short key
int32_t fk_common(const char *who, plk_ctx *ctx, uint32_t count, uint32_t log_n) {
    if (!fk_size_ok(log_n)) { set_error(std::string(who) + ": more than 2^25 points"); return PLK_ERR_SIZE; }
    if (!fk_batch_ok(count, log_n)) { set_error(std::string(who) + ": count x 2N exceeds 2^26 points (" + std::to_string(count) + " polynomials of 2^" + std::to_string(log_n) + ")"); return PLK_ERR_SIZE; }
    if (ctx->combine) { set_error(std::string(who) + ": single-GPU only (this context holds one shard of a key, plk_set_commit_shard)"); return PLK_ERR_ARG; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error(std::string(who) + ": a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    const uint64_t need = fk_key_points_needed(log_n), have = ctx->srs().pts ? ctx->srs().n : 0;
    if (!fk_key_ok(log_n, have)) {
        set_error(std::string(who) + ": the pass reads key points 0 .. N - 2: " + std::to_string(need) + " points needed, " + std::to_string(have) + " resident");
        return PLK_ERR_SRS;
    }
    return PLK_OK;
}

// DFT_2N(t) into ctx->fk_key unless it is there; *built = it was enqueued on st now (valid once st has been waited for)
int32_t fk_key_transform(plk_ctx *ctx, uint32_t log_n, hipStream_t st, bool *built) {
    *built = false;
    if (ctx->fk_key_valid && ctx->fk_key_log_n == log_n) return PLK_OK;
    ctx->fk_key_valid = false;
    if (fk_key_transform_bytes(log_n) > ctx->fk_key.cap) PLK_HIP(hipStreamSynchronize(st));
    PLK_TRY(ctx->fk_key.reserve(fk_key_transform_bytes(log_n)));
    XyzzW *t = ctx->fk_key.as<XyzzW>();
    const uint32_t n2 = 2u << log_n;
    hipLaunchKernelGGL(k_fk_arrange_t, dim3((n2 + 255) / 256), dim3(256), 0, st, t, static_cast<const G1Affine *>(ctx->srs().pts), log_n);
    PLK_HIP(hipGetLastError());
    PLK_TRY(g1_ntt_xyzzw_dev(ctx, t, 1, n2, log_n + 1, false, st));
    *built = true;
    return PLK_OK;
}

// `count` polynomials of N back to back (fk_batch_ok), proofs and evals likewise
int32_t open_all(plk_ctx *ctx, const Fr *poly, uint32_t count, uint32_t log_n, bool values, G1Affine *proofs, Fr *evals, hipStream_t st) {
    const uint32_t n = 1u << log_n, n2 = 2 * n;
    const size_t total = (size_t)count << log_n;                   // <= 2^25
    if (log_n == 0) {                                              // constants: the quotient is zero, its commitment the point at infinity
        PLK_HIP(hipMemsetAsync(proofs, 0, total * sizeof(G1Affine), st));
        if (evals) PLK_HIP(hipMemcpyAsync(evals, poly, total * sizeof(Fr), hipMemcpyDeviceToDevice, st));
        PLK_HIP(hipStreamSynchronize(st));
        return PLK_OK;
    }
    StageTimer<6> ev;
    PLK_TRY(ev.start(ctx));
    auto mark = [&](int k) { return ev.mark(k, st); };

    FkWs ws(ctx, st);
    const FkScratch lay = fk_batch_scratch(count, log_n, values);
    PLK_TRY(ws.reserve(lay.bytes));
    char *base = ctx->fk_ws.as<char>();
    XyzzW *u = reinterpret_cast<XyzzW *>(base + lay.u_off);
    Fr *c = reinterpret_cast<Fr *>(base + lay.c_off);

    PLK_TRY(mark(0));
    bool built = false;
    PLK_TRY(fk_key_transform(ctx, log_n, st, &built));
    PLK_TRY(mark(1));
    const Fr *f = poly;
    // the scalar transforms are 0.05 % of a pass: one ntt_dev per polynomial
    if (values) {                                                  // one inverse NTT into scratch: the input is never written, no Lagrange-form key is read
        Fr *coeffs = reinterpret_cast<Fr *>(base + lay.coeff_off);
        PLK_HIP(hipMemcpyAsync(coeffs, poly, total * sizeof(Fr), hipMemcpyDeviceToDevice, st));
        for (uint32_t b = 0; b < count; b++) PLK_TRY(ntt_dev(ctx, coeffs + ((size_t)b << log_n), log_n, true, nullptr, st));
        f = coeffs;
    }
    hipLaunchKernelGGL(k_fk_arrange_c, dim3((count * n2 + 255) / 256), dim3(256), 0, st, c, f, log_n, count);
    PLK_HIP(hipGetLastError());
    for (uint32_t b = 0; b < count; b++) PLK_TRY(ntt_dev(ctx, c + (size_t)b * n2, log_n + 1, false, nullptr, st));
    if (evals) {
        PLK_HIP(hipMemcpyAsync(evals, poly, total * sizeof(Fr), hipMemcpyDeviceToDevice, st));          // values: the answer itself
        if (!values) for (uint32_t b = 0; b < count; b++) PLK_TRY(ntt_dev(ctx, evals + ((size_t)b << log_n), log_n, false, nullptr, st));
    }
    PLK_TRY(mark(2));
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fk_pointwise), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO8));
        attr_set = true;
    }
    hipLaunchKernelGGL(k_fk_pointwise, dim3((count * n2 + G1NTT_THREADS - 1) / G1NTT_THREADS), dim3(G1NTT_THREADS), G1NTT_LDS_ISO8, st, u, (const Fr *)c,
                       (const XyzzW *)ctx->fk_key.as<XyzzW>(), count * n2, n2 - 1);
    PLK_HIP(hipGetLastError());
    PLK_TRY(mark(3));
    PLK_TRY(g1_ntt_xyzzw_dev(ctx, u, count, n2, log_n + 1, true, st));   // h_b = entries 0 .. N - 1 of block b; the upper halves are never read again
    PLK_TRY(mark(4));
    PLK_TRY(g1_ntt_xyzzw_dev(ctx, u, count, n2, log_n, false, st));
    PLK_TRY(g1_xyzzw_to_affine_dev(u, count, n2, log_n, proofs, st));    // gathers the first N of every 2N block into the dense proofs
    PLK_TRY(mark(5));
    PLK_HIP(hipStreamSynchronize(st));
    if (built) { ctx->fk_key_valid = true; ctx->fk_key_log_n = log_n; }
    if (ev.on) {
        for (int k = 0; k < 5; k++) PLK_TRY(ev.elapsed(k, k + 1, &ctx->fk_ms[k]));
        ctx->fk_ms_valid = true;
    }
    return PLK_OK;
}

}  // namespace
}  // namespace plk

using namespace plk;

extern "C" int32_t plk_kzg_open_all_prepare(plk_ctx *ctx, uint32_t log_n) {
    if (!ctx) { set_error("plk_kzg_open_all_prepare: bad argument"); return PLK_ERR_ARG; }
    PLK_TRY(fk_common("plk_kzg_open_all_prepare", ctx, 1, log_n));
    if (log_n == 0) return PLK_OK;                                 // no key point is read
    PLK_HIP(hipSetDevice(ctx->device));
    bool built = false;
    PLK_TRY(fk_key_transform(ctx, log_n, ctx->stream, &built));
    PLK_HIP(hipStreamSynchronize(ctx->stream));
    if (built) { ctx->fk_key_valid = true; ctx->fk_key_log_n = log_n; }
    return PLK_OK;
}

extern "C" int32_t plk_kzg_open_all_dev(plk_ctx *ctx, const void *poly_dev, uint32_t log_n, uint32_t flags, void *proofs_dev, void *evals_dev, void *stream) {
    const char *who = "plk_kzg_open_all_dev";
    if (!ctx || !poly_dev || !proofs_dev || (flags & ~(uint32_t)PLK_KZG_VALUES) || evals_dev == poly_dev) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    if (((uintptr_t)poly_dev | (uintptr_t)proofs_dev | (uintptr_t)evals_dev) & 15u) { set_error(std::string(who) + ": device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    ctx->fk_ms_valid = false;
    PLK_TRY(fk_common(who, ctx, 1, log_n));
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    return open_all(ctx, static_cast<const Fr *>(poly_dev), 1, log_n, (flags & PLK_KZG_VALUES) != 0, static_cast<G1Affine *>(proofs_dev), static_cast<Fr *>(evals_dev), st);
}

extern "C" int32_t plk_kzg_open_all_batch_dev(plk_ctx *ctx, const void *polys_dev, uint32_t count, uint32_t log_n, uint32_t flags, void *proofs_dev, void *evals_dev, void *stream) {
    const char *who = "plk_kzg_open_all_batch_dev";
    if (!ctx || !polys_dev || !proofs_dev || (flags & ~(uint32_t)PLK_KZG_VALUES) || evals_dev == polys_dev) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    if (count == 0) { set_error(std::string(who) + ": count must be at least 1"); return PLK_ERR_ARG; }
    if (((uintptr_t)polys_dev | (uintptr_t)proofs_dev | (uintptr_t)evals_dev) & 15u) { set_error(std::string(who) + ": device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    ctx->fk_ms_valid = false;
    PLK_TRY(fk_common(who, ctx, count, log_n));
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    return open_all(ctx, static_cast<const Fr *>(polys_dev), count, log_n, (flags & PLK_KZG_VALUES) != 0, static_cast<G1Affine *>(proofs_dev), static_cast<Fr *>(evals_dev), st);
}

extern "C" int32_t plk_kzg_open_all_last_ms(plk_ctx *ctx, float out_ms[5]) {
    if (!ctx || !out_ms) { set_error("plk_kzg_open_all_last_ms: bad argument"); return PLK_ERR_ARG; }
    if (!ctx->fk_ms_valid) { set_error("plk_kzg_open_all_last_ms: no timed plk_kzg_open_all_dev on this context (plk_set_kernel_timing)"); return PLK_ERR_ARG; }
    for (int k = 0; k < 5; k++) out_ms[k] = ctx->fk_ms[k];
    return PLK_OK;
}
