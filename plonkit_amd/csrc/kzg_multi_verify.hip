// Many multi-point openings (kzg_multi.hip; Boneh-Drake-Fisch-Gabizon 2020) verified on the device, each on its own: verdict i is what
// plk_kzg_verify_multi says about opening i.  No random combination across openings, no bisection.  NO COUNTERPART IN THE REFERENCE:
// bellman's kate_commitment opens at one point per call and checks one opening on one host thread.  Contracts: include/plonkit_amd.h.
//
// One shape (count, npoints, sets) serves the batch; per pass (kzg_multi_verify_plan.h: at most 2^16 openings and 64 MiB):
//   k_kmv_check    one opening per lane: range and curve checks, the pairwise distinctness of the points, the count + 3 scalars
//                  (kzg_multi_verify_dev.h: one inversion per opening, the running products in the pass buffer)        -> scalars, state
//   k_kmv_terms    one (opening, term) per lane, count + 3 times as many lanes: scalar x base by g1_mul_scalar_iso with the window
//                  table in LDS; a zero scalar, the identity or a malformed opening gives the identity without multiplying   -> products
//   k_kmv_sum      one opening per lane: the complete sum of its products (equal terms double, opposite terms cancel), A in affine
//                  form, B = -W'                                                                                        -> A, B
//   plk_pairing_check_many_dev's kernel on A and B, then k_kmv_settle: malformed openings get PLK_VERDICT_MALFORMED     -> verdicts
#include "ctx.h"
#include "ec_dev.h"
#include "ec29_dev.h"
#include "glv_dev.h"
#include "g1_mul_dev.h"
#include "pairing.h"
#include "g2_host.h"
#include "kzg_multi_plan.h"
#include "kzg_multi_verify_plan.h"
#include "kzg_multi_verify_dev.h"
#include <cstring>
#include <string>

namespace plk {

using host::KMV_BLOCK;
static_assert(KMV_BLOCK == G1NTT_THREADS, "the term kernel's window table is G1NTT_THREADS lanes wide");
static_assert(sizeof(XyzzW) == host::KMV_XYZZW_BYTES && sizeof(G1Affine) == host::KMV_AFFINE_BYTES && sizeof(Fr) == host::KMV_FR_BYTES, "the plan's sizes");
static_assert(host::KMV_MAX_OPEN == host::KM_MAX_OPEN && host::KMV_MAX_POINTS == host::KM_MAX_POINTS, "the shapes of plk_kzg_verify_multi");
static_assert(host::KMV_STATE_GOES_ON == FRONT_GOES_ON && host::KMV_STATE_MALFORMED == FRONT_MALFORMED, "the states of plk_verify_front_dev");

// the inputs of a pass: opening o owns count commitments, npoints points, count x npoints evaluations, gamma, u and two proof points
struct KmvInputs {
    const G1Affine *cm, *proofs;
    const Fr *pts, *ev, *gamma, *u;
};

// scalars[o * (count + 3) ..] and state[o]; run: the pass's running products, slot k of opening o at run[k * stride + o]
__global__ void __launch_bounds__(KMV_BLOCK) k_kmv_check(Fr *scalars, uint8_t *state, Fr *run, uint32_t stride, KmvShape S, KmvInputs in, uint32_t n) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    const size_t m = S.count, p = S.npoints;
    state[o] = (uint8_t)kmv_front(S, in.cm + o * m, in.pts + o * p, in.ev + o * m * p, in.gamma + o, in.u + o, in.proofs + 2 * (size_t)o, run + o, stride,
                                  scalars + o * (m + 3));
}

__device__ __forceinline__ XyzzW kmv_to_w(const G1Affine &a) {         // affine (2^256) -> XYZZ on the 29-bit layer (2^261); not for infinity
    XyzzW b;
    b.x = csub_p(w_from_s(unpack<FqW>(a.x))); b.y = csub_p(w_from_s(unpack<FqW>(a.y)));
    b.zz = w_one<FqW>(); b.zzz = w_one<FqW>();
    return b;
}

// products[lane] = scalar x base for lane = kmv_lane(opening, term); the identity where nothing is to be multiplied
__global__ void __launch_bounds__(G1NTT_THREADS, 1) k_kmv_terms(XyzzW *products, const Fr *scalars, const uint8_t *state, uint32_t count, KmvInputs in, uint32_t lanes) {
    extern __shared__ uint32_t g1tab[];
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= lanes) return;
    const uint32_t o = host::kmv_lane_opening(lane, count), t = host::kmv_lane_term(lane, count);
    XyzzW acc = xyzzw_identity();
    if (state[o] == host::KMV_STATE_GOES_ON) {
        const Fr k = load_fp(scalars + lane);
        G1Affine base;
        switch (host::kmv_term_base(t, count)) {
        case host::KMV_BASE_COMMITMENT: base = load_affine(in.cm + (size_t)o * count + t); break;
        case host::KMV_BASE_G: base.x = Fq::one(); base.y = add(base.x, base.x); break;           // the generator (1, 2)
        case host::KMV_BASE_W: base = load_affine(in.proofs + 2 * (size_t)o); break;
        default: base = load_affine(in.proofs + 2 * (size_t)o + 1); break;
        }
        if (!k.is_zero() && !is_inf(base)) acc = g1_mul_scalar_iso(kmv_to_w(base), to_canonical(k), g1tab);
    }
    store_xyzzw(products + lane, acc);
}

// A_o = the sum of the opening's count + 3 products as an affine point, B_o = -W'_o; (0, 0) twice for a malformed opening
__global__ void __launch_bounds__(KMV_BLOCK) k_kmv_sum(G1Affine *a_out, G1Affine *b_out, const XyzzW *products, const uint8_t *state, uint32_t count, const G1Affine *proofs, uint32_t n) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n) return;
    G1Affine A, B;
    A.x = Fq::zero(); A.y = Fq::zero(); B = A;
    if (state[o] == host::KMV_STATE_GOES_ON) {
        XyzzW acc = xyzzw_identity();
#pragma unroll 1
        for (uint32_t t = 0; t < host::kmv_terms(count); t++) {
            const XyzzW term = load_xyzzw(products + host::kmv_lane(o, t, count));
            g1_add_call(&acc, &term);                                  // the complete addition: doubles, cancels, passes the identity
        }
        const G1Xyzz s = xyzzw_export(acc);
        if (!is_inf(s)) {
            const Fq zi = inv(s.zzz), iz = mul(s.zz, zi), izz = mul(iz, iz);      // 1 / ZZZ, 1 / Z, 1 / ZZ
            A.x = mul(s.x, izz); A.y = mul(s.y, zi);
        }
        const G1Affine P = load_affine(proofs + 2 * (size_t)o + 1);
        B.x = P.x; B.y = neg(P.y);                                     // (infinity stays (0, 0))
    }
    store_fp(&a_out[o].x, A.x); store_fp(&a_out[o].y, A.y);
    store_fp(&b_out[o].x, B.x); store_fp(&b_out[o].y, B.y);
}

__global__ void __launch_bounds__(KMV_BLOCK) k_kmv_settle(uint8_t *verdict, const uint8_t *v, const uint8_t *state, uint32_t n) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o < n) verdict[o] = state[o] == host::KMV_STATE_GOES_ON ? v[o] : (uint8_t)PLK_VERDICT_MALFORMED;
}

namespace {
using namespace host;

struct KmvCall {
    const char *who;
    uint32_t count, npoints;
    const uint32_t *sets;
    const void *cm, *pts, *ev, *gamma, *u, *proofs;
    uint64_t n;
};

// what the host decides once, from the shape and the pointers
// (bytes_out: verdicts or states, any alignment; scalars_out: the front's scalars where the call has them)
int32_t kmv_check_call(plk_ctx *ctx, const KmvCall &c, const void *bytes_out, bool has_scalars_out, const void *scalars_out) {
    const std::string who = c.who;
    if (!ctx || !c.sets || (c.n && (!c.cm || !c.pts || !c.ev || !c.gamma || !c.u || !c.proofs || !bytes_out || (has_scalars_out && !scalars_out)))) {
        set_error(who + ": null argument"); return PLK_ERR_ARG; }
    HFr dummy[KM_MAX_POINTS];                                          // the sets alone are judged here; equal points are an opening's own business
    for (uint32_t j = 0; j < KM_MAX_POINTS; j++) dummy[j] = HFr::from_u64(j);
    const int verdict = km_check_sets(dummy, c.npoints, c.sets, c.count);
    if (verdict != KM_SETS_OK) { set_error(who + ": " + km_sets_words(verdict)); return PLK_ERR_ARG; }
    if (((uintptr_t)c.cm | (uintptr_t)c.pts | (uintptr_t)c.ev | (uintptr_t)c.gamma | (uintptr_t)c.u | (uintptr_t)c.proofs | (uintptr_t)scalars_out) & 15u) {
        set_error(who + ": device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    if (c.n > (1ull << 28)) { set_error(who + ": more than 2^28 openings"); return PLK_ERR_SIZE; }
    return PLK_OK;
}

KmvShape kmv_shape(const KmvCall &c) {
    KmvShape S;
    memset(&S, 0, sizeof S);
    S.count = c.count; S.npoints = c.npoints;
    memcpy(S.sets, c.sets, c.count * sizeof(uint32_t));
    return S;
}
KmvInputs kmv_inputs(const KmvCall &c, uint64_t base) {
    KmvInputs in;
    in.cm = static_cast<const G1Affine *>(c.cm) + base * c.count;
    in.proofs = static_cast<const G1Affine *>(c.proofs) + base * 2;
    in.pts = static_cast<const Fr *>(c.pts) + base * c.npoints;
    in.ev = static_cast<const Fr *>(c.ev) + base * c.count * c.npoints;
    in.gamma = static_cast<const Fr *>(c.gamma) + base;
    in.u = static_cast<const Fr *>(c.u) + base;
    return in;
}
}  // namespace
}  // namespace plk

using namespace plk;

extern "C" int32_t plk_kzg_verify_multi_front_dev(plk_ctx *ctx, uint32_t count, uint32_t npoints, const uint32_t *sets, const void *commitments_dev, const void *points_dev,
                                                  const void *evals_dev, const void *gamma_dev, const void *u_dev, const void *proofs_dev, uint64_t n, void *scalars_dev,
                                                  void *state_dev, void *stream) {
    const KmvCall c{"plk_kzg_verify_multi_front_dev", count, npoints, sets, commitments_dev, points_dev, evals_dev, gamma_dev, u_dev, proofs_dev, n};
    PLK_TRY(kmv_check_call(ctx, c, state_dev, true, scalars_dev));
    if (ctx->msm_enq != ctx->msm_fin) { set_error(std::string(c.who) + ": a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    const uint64_t pass = host::kmv_pass(count, npoints), m = n < pass ? n : pass;
    PLK_TRY(ctx->kzg_vm.reserve(host::kmv_front_bytes(npoints, m) + 16));          // (+ 16: one point has no pairs, and a buffer must exist)
    Fr *run = ctx->kzg_vm.as<Fr>();
    const KmvShape S = kmv_shape(c);
    return on_ctx_stream(ctx, stream ? (hipStream_t)stream : ctx->stream, [&](hipStream_t st) -> int32_t {
        for (uint64_t base = 0; base < n; base += pass) {
            const uint32_t cnt = (uint32_t)(n - base < pass ? n - base : pass);
            hipLaunchKernelGGL(k_kmv_check, dim3(host::kmv_blocks(cnt)), dim3(KMV_BLOCK), 0, st, static_cast<Fr *>(scalars_dev) + base * host::kmv_terms(count),
                               static_cast<uint8_t *>(state_dev) + base, run, (uint32_t)m, S, kmv_inputs(c, base), cnt);
            PLK_HIP(hipGetLastError());
        }
        return PLK_OK;
    });
}

extern "C" int32_t plk_kzg_verify_multi_many_dev(plk_ctx *ctx, uint32_t count, uint32_t npoints, const uint32_t *sets, const void *commitments_dev, const void *points_dev,
                                                 const void *evals_dev, const void *gamma_dev, const void *u_dev, const void *proofs_dev, uint64_t n, const uint8_t g2[256],
                                                 void *verdict_dev, void *stream) {
    const KmvCall c{"plk_kzg_verify_multi_many_dev", count, npoints, sets, commitments_dev, points_dev, evals_dev, gamma_dev, u_dev, proofs_dev, n};
    if (!g2) { set_error(std::string(c.who) + ": null argument"); return PLK_ERR_ARG; }
    PLK_TRY(kmv_check_call(ctx, c, verdict_dev, false, nullptr));
    host::G2Affine q[2];
    if (!host::g2_from_bytes(g2, &q[0]) || !host::g2_from_bytes(g2 + 128, &q[1])) { set_error("plk_pairing_check: G2 point not on the twist"); return PLK_ERR_ARG; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error(std::string(c.who) + ": a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    // the call does not wait: a buffer of its own and the context's stream (on_ctx_stream, ctx.h)
    const uint64_t pass = host::kmv_pass(count, npoints), m = n < pass ? n : pass;
    const host::KmvLayout L = host::kmv_layout(count, npoints, m);
    PLK_TRY(ctx->kzg_vm.reserve(L.total));
    char *d = ctx->kzg_vm.as<char>();
    Fr *scalars = reinterpret_cast<Fr *>(d + L.scalars), *run = reinterpret_cast<Fr *>(d + L.run);
    XyzzW *products = reinterpret_cast<XyzzW *>(d + L.products);
    G1Affine *a = reinterpret_cast<G1Affine *>(d + L.a), *b = reinterpret_cast<G1Affine *>(d + L.b);
    uint8_t *vv = reinterpret_cast<uint8_t *>(d + L.verdict), *state = reinterpret_cast<uint8_t *>(d + L.state);
    const KmvShape S = kmv_shape(c);
    return on_ctx_stream(ctx, stream ? (hipStream_t)stream : ctx->stream, [&](hipStream_t st) -> int32_t {
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_kmv_terms), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO));
        for (uint64_t base = 0; base < n; base += pass) {
            const uint32_t cnt = (uint32_t)(n - base < pass ? n - base : pass), lanes = (uint32_t)host::kmv_lanes(cnt, count);
            const KmvInputs in = kmv_inputs(c, base);
            hipLaunchKernelGGL(k_kmv_check, dim3(host::kmv_blocks(cnt)), dim3(KMV_BLOCK), 0, st, scalars, state, run, (uint32_t)m, S, in, cnt);
            hipLaunchKernelGGL(k_kmv_terms, dim3(host::kmv_blocks(lanes)), dim3(G1NTT_THREADS), G1NTT_LDS_ISO, st, products, (const Fr *)scalars, (const uint8_t *)state, count, in, lanes);
            hipLaunchKernelGGL(k_kmv_sum, dim3(host::kmv_blocks(cnt)), dim3(KMV_BLOCK), 0, st, a, b, (const XyzzW *)products, (const uint8_t *)state, count, in.proofs, cnt);
            PLK_HIP(hipGetLastError());
            PLK_TRY(plk_pairing_check_many_dev(ctx, a, b, cnt, g2, vv, st));
            hipLaunchKernelGGL(k_kmv_settle, dim3(host::kmv_blocks(cnt)), dim3(KMV_BLOCK), 0, st, static_cast<uint8_t *>(verdict_dev) + base, (const uint8_t *)vv, (const uint8_t *)state, cnt);
            PLK_HIP(hipGetLastError());
        }
        return PLK_OK;
    });
}
