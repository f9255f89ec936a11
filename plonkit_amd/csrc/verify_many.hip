// Many proofs of one verification key, each verified exactly and on its own (plk_vk_load, plk_verify_many, plk_pairing_check_many_dev).
// NO COUNTERPART IN THE REFERENCE, whose plonk::verify (src/plonk.rs:189-210) takes one proof on one host thread; verdict i is what
// plk_verify_ex says about proof i.  There is no random linear combination across proofs and no shared pairing.
//
// Host, per proof, on up to 16 threads: parse, transcript, the scalar checks, and the flattened scalars of verify.cpp (plk_verify_terms).
// Device, for the proofs that pass that:
//   vm_mul_kernel      one (proof, term) per lane, 25 terms per proof: the GLV double-and-add of g1_mul_dev.h with four effectively affine
//                      table entries (g1_mul_scalar_iso: 72 KB of LDS per 256 lanes, two workgroups per CU)
//   vm_sum_kernel      one lane per (proof, side): 23 -> 1 and 2 -> 1 on the 29-bit layer, left as XYZZ in the external form
//   vm_affine_kernel   XYZZ -> affine, one inversion per 8 points (as srs_to_affine_kernel); infinity comes out as x = y = 0
//   vm_pairing_kernel  one proof per lane: f <- f^2 l_0 l_1 over the uploaded line table, then the shortened final exponentiation of
//                      fq12_dev.h (which decides the same predicate as pairing.cpp's; the argument is written there)
#include "ctx.h"
#include "ec_dev.h"
#include "ec29_dev.h"
#include "glv_dev.h"
#include "g1_mul_dev.h"
#include "fq12_dev.h"
#include "pairing_table.h"
#include "verify_many.h"
#include "circuit.h"
#include <atomic>
#include <chrono>
#include <cstring>

namespace plk {

constexpr uint32_t VM_PROOF_PTS = 11;                              // points a proof brings: wires 4, grand product, quotient 4, W_z, W_zw
constexpr uint32_t VM_NORM_K = 8;
constexpr uint32_t VM_PAIR_THREADS = 64;                           // one wave per workgroup: a small batch still spreads over the CUs
constexpr uint64_t VM_CHUNK = 1u << 16;                            // proofs per pass through the staging arena (5.5 KB each)

// term t of proof p: 0..10 the key's commitments and 22 the generator (fixed[0..11]); 11..21 the proof's points; 23, 24 = W_z, W_zw again
__device__ __forceinline__ const G1Affine *vm_term_point(const G1Affine *fixed, const G1Affine *pts, uint32_t p, uint32_t t) {
    if (t < 11) return fixed + t;
    if (t < 22) return pts + (size_t)p * VM_PROOF_PTS + (t - 11);
    if (t == 22) return fixed + 11;
    return pts + (size_t)p * VM_PROOF_PTS + (t - 23 + 9);
}

__global__ void __launch_bounds__(G1NTT_THREADS, 1) vm_mul_kernel(XyzzW *prod, const G1Affine *fixed, const G1Affine *pts, const Fr *sc, uint32_t m) {
    extern __shared__ uint32_t g1tab[];
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m * (uint32_t)VERIFY_TERMS) return;
    const uint32_t p = j / VERIFY_TERMS, t = j % VERIFY_TERMS;
    const G1Affine a = load_affine(vm_term_point(fixed, pts, p, t));
    XyzzW b = xyzzw_identity();
    if (!is_inf(a)) {
        b.x = csub_p(w_from_s(unpack<FqW>(a.x))); b.y = csub_p(w_from_s(unpack<FqW>(a.y)));
        b.zz = w_one<FqW>(); b.zzz = w_one<FqW>();
    }
    const Fr k = to_canonical(load_fp(sc + j));                   // the header's scalars are canonical, the ABI's are Montgomery
    store_xyzzw(prod + j, g1_mul_scalar_iso(b, k, g1tab));
}

__global__ void __launch_bounds__(256) vm_sum_kernel(G1Xyzz *sums, const XyzzW *prod, uint32_t m) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * m) return;
    const uint32_t p = j >> 1, lo = (j & 1) ? VERIFY_TERMS_PG : 0, hi = (j & 1) ? VERIFY_TERMS : VERIFY_TERMS_PG;
    const XyzzW *src = prod + (size_t)p * VERIFY_TERMS;
    XyzzW acc = load_xyzzw(src + lo);
    for (uint32_t k = lo + 1; k < hi; k++) { const XyzzW b = load_xyzzw(src + k); g1_add_call(&acc, &b); }
    store_xyzz(sums + j, xyzzw_export(acc));
}

__global__ void __launch_bounds__(256) vm_affine_kernel(G1Affine *out, const G1Xyzz *in, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lo = t * VM_NORM_K, hi = lo + VM_NORM_K < n ? lo + VM_NORM_K : n;
    if (lo >= n) return;
    Fq prefix[VM_NORM_K];
    Fq acc = Fq::one();
#pragma unroll
    for (uint32_t j = 0; j < VM_NORM_K; j++) {
        if (lo + j < hi) { const Fq z = load_fp(&in[lo + j].zzz); if (!z.is_zero()) acc = mul(acc, z); }
        prefix[j] = acc;
    }
    Fq inv_acc = inv(acc);
#pragma unroll
    for (uint32_t jj = 0; jj < VM_NORM_K; jj++) {
        const uint32_t j = VM_NORM_K - 1 - jj;
        if (lo + j >= hi) continue;
        const G1Xyzz q = load_xyzz(in + lo + j);
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

// verdict[i] = 1 / 0: e(a_i, Q0) e(b_i, Q1) is / is not 1;  2: a_i or b_i is not on the curve.  a_i = a[i * stride], b_i = b[i * stride]
__global__ void __launch_bounds__(VM_PAIR_THREADS) vm_pairing_kernel(uint8_t *verdict, const G1Affine *a, const G1Affine *b, uint32_t stride, uint32_t n,
                                                                     const PairingHead *head, const Fq *lines) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Affine A = load_affine(a + (size_t)i * stride), B = load_affine(b + (size_t)i * stride);
    uint8_t v = 2;
    if (fq_on_curve(A.x, A.y) && fq_on_curve(B.x, B.y)) v = pairing_is_one_from_lines(A.x, A.y, B.x, B.y, head, lines) ? 1 : 0;
    verdict[i] = v;
}

// [PairingHead | lines | fixed points] in one device allocation
static size_t table_bytes(uint32_t lines) { return sizeof(PairingHead) + (size_t)lines * 8 * sizeof(Fq); }
static_assert(sizeof(PairingHead) % 16 == 0, "the line table behind the head must stay 16-byte aligned");

static int32_t pairing_launch(uint8_t *verdict, const G1Affine *a, const G1Affine *b, uint32_t stride, uint32_t n, const void *table, hipStream_t st) {
    const PairingHead *head = reinterpret_cast<const PairingHead *>(table);
    const Fq *lines = reinterpret_cast<const Fq *>(reinterpret_cast<const char *>(table) + sizeof(PairingHead));
    hipLaunchKernelGGL(vm_pairing_kernel, dim3((n + VM_PAIR_THREADS - 1) / VM_PAIR_THREADS), dim3(VM_PAIR_THREADS), 0, st, verdict, a, b, stride, n, head, lines);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

}  // namespace plk

using namespace plk;

struct plk_vk {
    int device = 0;
    uint32_t flags = 0;
    ParsedVk *parsed = nullptr;
    void *dev = nullptr;                                           // [PairingHead | lines | 12 fixed points]
    size_t fixed_off = 0;
};

extern "C" void plk_vk_free(plk_vk *vk) {
    if (!vk) return;
    if (vk->dev) { (void)hipSetDevice(vk->device); (void)hipFree(vk->dev); }
    parsed_vk_free(vk->parsed);
    delete vk;
}

extern "C" int32_t plk_vk_load(plk_ctx *ctx, const uint8_t *vk_bytes, uint64_t len, uint32_t flags, plk_vk **out) {
    if (!ctx || !vk_bytes || !out) { set_error("plk_vk_load: null argument"); return PLK_ERR_ARG; }
    if (flags & ~(uint32_t)PLK_VERIFY_STRICT_INPUTS) { set_error("plk_verify_ex: unknown flag"); return PLK_ERR_ARG; }
    ParsedVk *parsed = parsed_vk_new(vk_bytes, len);
    if (!parsed) { set_error("plk_verify: malformed verification key"); return PLK_ERR_ARG; }
    plk_vk *vk = new plk_vk;
    vk->device = ctx->device; vk->flags = flags; vk->parsed = parsed;
    plk_g1_affine fixed[VERIFY_FIXED]; host::G2Affine g2[2];
    parsed_vk_points(parsed, fixed, g2);
    PairingHead head; std::vector<Fq> lines;
    make_pairing_table(g2, &head, &lines);
    vk->fixed_off = table_bytes(head.lines);
    std::vector<uint8_t> img(vk->fixed_off + sizeof fixed);
    memcpy(img.data(), &head, sizeof head);
    memcpy(img.data() + sizeof head, lines.data(), lines.size() * sizeof(Fq));
    memcpy(img.data() + vk->fixed_off, fixed, sizeof fixed);
    int32_t rc = [&]() -> int32_t {
        PLK_HIP(hipSetDevice(ctx->device));
        PLK_HIP(hipMalloc(&vk->dev, img.size()));
        PLK_HIP(hipMemcpy(vk->dev, img.data(), img.size(), hipMemcpyHostToDevice));
        return PLK_OK;
    }();
    if (rc != PLK_OK) { plk_vk_free(vk); return rc; }
    *out = vk;
    return PLK_OK;
}

extern "C" int32_t plk_pairing_check_many_dev(plk_ctx *ctx, const void *a_dev, const void *b_dev, uint64_t n, const uint8_t g2[256], void *verdict_dev, void *stream) {
    if (!ctx || !g2 || (n && (!a_dev || !b_dev || !verdict_dev))) { set_error("plk_pairing_check_many_dev: null argument"); return PLK_ERR_ARG; }
    if (((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)verdict_dev) & 15) { set_error("plk_pairing_check_many_dev: device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    if (n > (1ull << 28)) { set_error("plk_pairing_check_many_dev: more than 2^28 checks"); return PLK_ERR_SIZE; }
    host::G2Affine q[2];
    if (!host::g2_from_bytes(g2, &q[0]) || !host::g2_from_bytes(g2 + 128, &q[1])) { set_error("plk_pairing_check: G2 point not on the twist"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (!ctx->pair_tab_valid || memcmp(ctx->pair_g2, g2, 256) != 0) {
        // a new G2 pair: its table replaces the last one's, which kernels already on `st` may still read
        PairingHead head; std::vector<Fq> lines;
        make_pairing_table(q, &head, &lines);
        std::vector<uint8_t> img(table_bytes(head.lines));
        memcpy(img.data(), &head, sizeof head);
        memcpy(img.data() + sizeof head, lines.data(), lines.size() * sizeof(Fq));
        ctx->pair_tab_valid = false;
        PLK_HIP(hipStreamSynchronize(st));
        PLK_TRY(ctx->pair_tab.reserve(img.size()));
        PLK_HIP(hipMemcpy(ctx->pair_tab.p, img.data(), img.size(), hipMemcpyHostToDevice));
        memcpy(ctx->pair_g2, g2, 256);
        ctx->pair_tab_valid = true;
    }
    return pairing_launch(reinterpret_cast<uint8_t *>(verdict_dev), reinterpret_cast<const G1Affine *>(a_dev), reinterpret_cast<const G1Affine *>(b_dev), 1, (uint32_t)n,
                          ctx->pair_tab.p, st);
}

static int32_t verify_many_impl(plk_ctx *ctx, const plk_vk *vk, const uint8_t *const *proofs, const uint64_t *lens, uint64_t count, uint8_t *verdict) {
    using clk = std::chrono::steady_clock;
    const bool timed = ctx->ev_on;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 6; k++) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
    ctx->vm_ms_valid = false;
    float ms[6] = {0, 0, 0, 0, 0, 0};
    hipStream_t st = ctx->stream;
    if (timed) for (int k = 0; k < 6; k++) PLK_HIP(hipEventCreate(&ev[k]));
    auto mark = [&](int k) -> int32_t { if (timed) PLK_HIP(hipEventRecord(ev[k], st)); return PLK_OK; };
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vm_mul_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO));
        attr_set = true;
    }
    std::vector<plk_g1_affine> h_pts;
    std::vector<plk_fr> h_sc;
    std::vector<uint64_t> live;
    std::vector<uint8_t> h_v;
    for (uint64_t base = 0; base < count; base += VM_CHUNK) {
        const uint64_t cnt = count - base < VM_CHUNK ? count - base : VM_CHUNK;
        // host: every proof of the chunk through plk_verify_terms's code; the survivors are packed in index order
        const auto t0 = clk::now();
        std::vector<plk_g1_affine> all_pts((size_t)cnt * VM_PROOF_PTS);
        std::vector<plk_fr> all_sc((size_t)cnt * VERIFY_TERMS);
        parallel_for((size_t)cnt, 1, [&](size_t lo, size_t hi) {
            plk_g1_affine pts[VERIFY_TERMS]; plk_fr sc[VERIFY_TERMS];
            for (size_t i = lo; i < hi; i++) {
                int32_t early = 0;
                const int32_t rc = verify_terms_parsed(vk->parsed, proofs[base + i], lens[base + i], vk->flags, pts, sc, &early);
                if (rc != PLK_OK) { verdict[base + i] = PLK_VERDICT_MALFORMED; continue; }
                if (!early) { verdict[base + i] = 0; continue; }
                verdict[base + i] = 0xff;                             // goes to the device
                memcpy(&all_pts[i * VM_PROOF_PTS], &pts[11], VM_PROOF_PTS * sizeof(plk_g1_affine));
                memcpy(&all_sc[i * VERIFY_TERMS], sc, sizeof sc);
            }
        }, 16);
        live.clear();
        for (uint64_t i = 0; i < cnt; i++) if (verdict[base + i] == 0xff) live.push_back(i);
        const uint32_t m = (uint32_t)live.size();
        h_pts.resize((size_t)m * VM_PROOF_PTS); h_sc.resize((size_t)m * VERIFY_TERMS); h_v.resize(m);
        for (uint32_t k = 0; k < m; k++) {
            memcpy(&h_pts[(size_t)k * VM_PROOF_PTS], &all_pts[live[k] * VM_PROOF_PTS], VM_PROOF_PTS * sizeof(plk_g1_affine));
            memcpy(&h_sc[(size_t)k * VERIFY_TERMS], &all_sc[live[k] * VERIFY_TERMS], VERIFY_TERMS * sizeof(plk_fr));
        }
        ms[0] += std::chrono::duration<float, std::milli>(clk::now() - t0).count();
        if (!m) continue;
        // device: the staging arena holds points | scalars | products | sums | affine pairs | verdict bytes, every part 16-byte aligned
        const size_t b_pts = (size_t)m * VM_PROOF_PTS * sizeof(G1Affine), b_sc = (size_t)m * VERIFY_TERMS * sizeof(Fr), b_prod = (size_t)m * VERIFY_TERMS * sizeof(XyzzW),
                     b_sum = (size_t)m * 2 * sizeof(G1Xyzz), b_aff = (size_t)m * 2 * sizeof(G1Affine), b_v = ((size_t)m + 15) & ~(size_t)15;
        PLK_TRY(ctx->stage.reserve(b_pts + b_sc + b_prod + b_sum + b_aff + b_v));
        char *d = ctx->stage.as<char>();
        G1Affine *d_pts = reinterpret_cast<G1Affine *>(d);
        Fr *d_sc = reinterpret_cast<Fr *>(d + b_pts);
        XyzzW *d_prod = reinterpret_cast<XyzzW *>(d + b_pts + b_sc);
        G1Xyzz *d_sum = reinterpret_cast<G1Xyzz *>(d + b_pts + b_sc + b_prod);
        G1Affine *d_aff = reinterpret_cast<G1Affine *>(d + b_pts + b_sc + b_prod + b_sum);
        uint8_t *d_v = reinterpret_cast<uint8_t *>(d + b_pts + b_sc + b_prod + b_sum + b_aff);
        const G1Affine *d_fixed = reinterpret_cast<const G1Affine *>(reinterpret_cast<const char *>(vk->dev) + vk->fixed_off);
        PLK_TRY(mark(0));
        PLK_HIP(hipMemcpyAsync(d_pts, h_pts.data(), b_pts, hipMemcpyHostToDevice, st));
        PLK_HIP(hipMemcpyAsync(d_sc, h_sc.data(), b_sc, hipMemcpyHostToDevice, st));
        PLK_TRY(mark(1));
        const uint32_t lanes = m * (uint32_t)VERIFY_TERMS;
        hipLaunchKernelGGL(vm_mul_kernel, dim3((lanes + G1NTT_THREADS - 1) / G1NTT_THREADS), dim3(G1NTT_THREADS), G1NTT_LDS_ISO, st, d_prod, d_fixed, (const G1Affine *)d_pts,
                           (const Fr *)d_sc, m);
        PLK_HIP(hipGetLastError());
        PLK_TRY(mark(2));
        hipLaunchKernelGGL(vm_sum_kernel, dim3((2 * m + 255) / 256), dim3(256), 0, st, d_sum, (const XyzzW *)d_prod, m);
        hipLaunchKernelGGL(vm_affine_kernel, dim3(((2 * m + VM_NORM_K - 1) / VM_NORM_K + 255) / 256), dim3(256), 0, st, d_aff, (const G1Xyzz *)d_sum, 2 * m);
        PLK_HIP(hipGetLastError());
        PLK_TRY(mark(3));
        PLK_TRY(pairing_launch(d_v, d_aff, d_aff + 1, 2, m, vk->dev, st));
        PLK_TRY(mark(4));
        PLK_HIP(hipMemcpyAsync(h_v.data(), d_v, m, hipMemcpyDeviceToHost, st));
        PLK_TRY(mark(5));
        PLK_HIP(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < m; k++) verdict[base + live[k]] = h_v[k];
        if (timed) for (int k = 0; k < 5; k++) { float t = 0; PLK_HIP(hipEventElapsedTime(&t, ev[k], ev[k + 1])); ms[k + 1] += t; }
    }
    if (timed) { memcpy(ctx->vm_ms, ms, sizeof ms); ctx->vm_ms_valid = true; }
    return PLK_OK;
}

extern "C" int32_t plk_verify_many(plk_ctx *ctx, const plk_vk *vk, const uint8_t *const *proofs, const uint64_t *lens, uint64_t count, uint8_t *verdict, uint64_t *first_bad) {
    if (!ctx || !vk || !verdict || !first_bad || (count && (!proofs || !lens))) { set_error("plk_verify_many: null argument"); return PLK_ERR_ARG; }
    for (uint64_t i = 0; i < count; i++) if (!proofs[i]) { set_error("plk_verify_many: null argument"); return PLK_ERR_ARG; }
    if (vk->device != ctx->device) { set_error("plk_verify_many: the verification key was loaded on another device"); return PLK_ERR_ARG; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error("plk_verify_many: a commitment enqueued with plk_msm_g1_enqueue_dev is still in flight (call plk_msm_g1_finish first)"); return PLK_ERR_ARG; }
    *first_bad = UINT64_MAX;
    if (count == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    int32_t rc = PLK_ERR_HIP;
    try { rc = verify_many_impl(ctx, vk, proofs, lens, count, verdict); }
    catch (const std::exception &e) { set_error(std::string("plk_verify_many: ") + e.what()); return PLK_ERR_ARG; }
    if (rc != PLK_OK) return rc;
    for (uint64_t i = 0; i < count; i++) if (verdict[i] != 1) { *first_bad = i; break; }
    return PLK_OK;
}

extern "C" int32_t plk_verify_many_last_ms(plk_ctx *ctx, float out_ms[6]) {
    if (!ctx || !out_ms) { set_error("plk_verify_many_last_ms: null argument"); return PLK_ERR_ARG; }
    if (!ctx->vm_ms_valid) { set_error("plk_verify_many_last_ms: no timed plk_verify_many on this context (plk_set_kernel_timing)"); return PLK_ERR_ARG; }
    for (int k = 0; k < 6; k++) out_ms[k] = ctx->vm_ms[k];
    return PLK_OK;
}
