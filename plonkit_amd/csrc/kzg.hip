// KZG openings on their own: commit, open at a point (from coefficients or from the values on the domain), verify one opening on the host
// and many on the device.  bellman's kate_commitment module (reached from src/plonk.rs:4) has commit_using_monomials, commit_using_values,
// open_from_monomials, open_from_values and is_valid_opening; the prover runs the same steps inside round 5.  Contracts: include/plonkit_amd.h.
//
// THE VALUES ROUTE needs 1 / (omega^i - z) for all i < N.  As in the grand product (prover.hip) there is no per-element inversion:
//   k_kzg_denoms     d_i = omega^i - z from the context's omega table, written twice (the two scans run in place)
//   scan_pair_mult   A_i = prod_{j<i} d_j and B_i = prod_{j>i} d_j, block-local; the block prefixes are folded in by the consumers
//   host             ONE inversion of the grand total
//   k_kzg_sum_partial / k_kzg_sum_finish    sum_i (f_i - y) omega^i / (omega^i - z): the barycentric sum (y = 0) and the in-domain position
//   k_kzg_div        q_i = (f_i - y) / (omega^i - z)
// z = omega^k: the host decides z^N = 1; k_kzg_denoms<true> then replaces the one vanishing denominator by 1 (a zero would make every
// product zero) and reports k, found by comparing the canonical difference limb for limb in the lane that owns it.  f(z) is read from
// the array, and position k of the quotient is q(omega^k) = sum_{i != k} (f_i - y) omega^i / (z (z - omega^i)), the value there of the
// polynomial quotient of degree < N - 1.
// Domains (poly.h): vectors and scalars carry 2^256 (E); the scans and the omega table live in the 2^261 domain (W); a product of the
// 29-bit layer removes 2^261, so W x W = W and W x E = E.
#include "ctx.h"
#include "msm.h"
#include "poly.h"
#include "ntt.h"
#include "ec_dev.h"
#include "ec29_dev.h"
#include "glv_dev.h"
#include "g1_mul_dev.h"
#include "fq12_dev.h"
#include "field29_dev.h"
#include "prover_math.h"
#include "pairing.h"
#include "g2_host.h"
#include "kzg_scratch.h"
#include <cstring>
#include <string>

namespace plk {

constexpr int KZ_T = 256;                                       // threads per block
constexpr int KZ_E = 8;                                         // elements per thread of the reductions
constexpr uint32_t KZ_BLOCK = KZ_T * KZ_E;
static_assert(KZ_BLOCK == POLY_SCAN_BLOCK, "the consumers fold in the scan's block prefixes: same block size");
constexpr uint32_t KZ_MAX = 8;                                  // polynomials per call
constexpr uint32_t KZ_NONE = 0xffffffffu;
constexpr uint64_t KZ_VM_CHUNK = 1u << 16;                      // openings per pass of plk_kzg_verify_many_dev

__device__ __forceinline__ FrW9 kz_ldw(const Fr *p) { return unpack<FrW>(load_fp(p)); }
__device__ __forceinline__ FrW9 kz_omega_w(const PowTable &t, uint32_t e) { return mulw(kz_ldw(t.lo + (e & (POW_TAB - 1))), kz_ldw(t.hi + (e >> POW_SPLIT))); }

// a[i] = b[i] = W(omega^i - z), canonical.  IN: the lane whose difference vanishes stores W(1) instead and reports its index.
template <bool IN>
__global__ void __launch_bounds__(KZ_T) k_kzg_denoms(Fr *a, Fr *b, PowTable tw, Fr z_w, uint32_t n, uint32_t shift, uint32_t *k_out) {
    const uint32_t i = blockIdx.x * KZ_T + threadIdx.x;
    if (i >= n) return;
    FrW9 d = reduce_small(sub2(kz_omega_w(tw, i << shift), unpack<FrW>(z_w)));
    if (IN && w_all_zero(d)) { d = w_one<FrW>(); *k_out = i; }
    const Fr v = pack<FrParams>(d);
    store_fp(a + i, v);
    store_fp(b + i, v);
}

// what the consumers need of the two scans: A = exclusive prefix products, B = exclusive suffix products (block-local), their block
// prefixes in scan order (null: one block), and s_w = W(1 / prod d_i)
struct KzgInv {
    const Fr *A, *B, *preA, *preB;
    Fr s_w;
    uint32_t n;
};
// W(1 / (omega^i - z))
__device__ __forceinline__ FrW9 kz_inverse(const KzgInv &v, uint32_t i) {
    FrW9 a = kz_ldw(v.A + i), b = kz_ldw(v.B + i);
    if (v.preA) { a = mulw(a, kz_ldw(v.preA + i / KZ_BLOCK)); b = mulw(b, kz_ldw(v.preB + (v.n - 1 - i) / KZ_BLOCK)); }
    return mulw(mulw(a, b), unpack<FrW>(v.s_w));
}

// partial[j * gridDim.x + block] = sum over the block's i != skip of (f_j[i] - y) * omega^i / (omega^i - z)      (E, canonical)
struct KzgPolys { const Fr *f[KZ_MAX]; };
__global__ void __launch_bounds__(KZ_T) k_kzg_sum_partial(Fr *partials, KzgPolys P, KzgInv v, PowTable tw, uint32_t shift, Fr y, uint32_t skip) {
    __shared__ __attribute__((aligned(16))) Fr sh[KZ_T];
    const uint32_t tid = threadIdx.x, j = blockIdx.y;
    const Fr *f = P.f[j];
    Fr acc = Fr::zero();
#pragma unroll 1
    for (int e = 0; e < KZ_E; e++) {
        const uint32_t i = blockIdx.x * KZ_BLOCK + e * KZ_T + tid;
        if (i >= v.n || i == skip) continue;
        const FrW9 wi = mulw(kz_inverse(v, i), kz_omega_w(tw, i << shift));
        acc = add(acc, pack<FrParams>(csub_p(mulw(wi, unpack<FrW>(sub(load_fp(f + i), y))))));
    }
    sh[tid] = acc;
    __syncthreads();
    for (int off = KZ_T / 2; off > 0; off >>= 1) {
        if ((int)tid < off) { acc = add(acc, sh[tid + off]); sh[tid] = acc; }
        __syncthreads();
    }
    if (tid == 0) store_fp(partials + (size_t)j * gridDim.x + blockIdx.x, acc);
}
__global__ void __launch_bounds__(KZ_T) k_kzg_sum_finish(Fr *results, const Fr *partials, uint32_t nb) {
    __shared__ __attribute__((aligned(16))) Fr sh[KZ_T];
    const uint32_t tid = threadIdx.x, j = blockIdx.x;
    Fr acc = Fr::zero();
    for (uint32_t b = tid; b < nb; b += KZ_T) acc = add(acc, load_fp(partials + (size_t)j * nb + b));
    sh[tid] = acc;
    __syncthreads();
    for (int off = KZ_T / 2; off > 0; off >>= 1) {
        if ((int)tid < off) { acc = add(acc, sh[tid + off]); sh[tid] = acc; }
        __syncthreads();
    }
    if (tid == 0) store_fp(results + j, acc);
}

// q[i] = (f[i] - y) / (omega^i - z), canonical; position `skip` is left to the caller (in-domain).  q may be f: a lane reads its element first.
__global__ void __launch_bounds__(KZ_T) k_kzg_div(Fr *q, const Fr *f, KzgInv v, Fr y, uint32_t skip) {
    const uint32_t i = blockIdx.x * KZ_T + threadIdx.x;
    if (i >= v.n || i == skip) return;
    const FrW9 d = unpack<FrW>(sub(load_fp(f + i), y));
    store_fp(q + i, pack<FrParams>(csub_p(mulw(kz_inverse(v, i), d))));
}

// ---- the front of plk_kzg_verify_many_dev: one opening per lane.  A = C + z pi + (-y) G, B = -pi, in the layout the pairing kernel reads.
// k_kzg_vm_check flags malformed openings, k_kzg_vm_front does the two multiplications and the sum, k_kzg_vm_finish the affine form,
// k_kzg_vm_settle writes the verdict bytes behind the pairing kernel.
__device__ __forceinline__ bool kz_fr_below_modulus(const Fr &v) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)v.l[i] - FrParams::P[i] - br; br = (d >> 32) & 1; }
    return br != 0;
}
__device__ __forceinline__ bool kz_point_ok(const G1Affine &p) {
    return fq_below_modulus(p.x) && fq_below_modulus(p.y) && fq_on_curve(p.x, p.y);          // (0, 0) is infinity
}
__device__ __forceinline__ XyzzW kz_to_w(const G1Affine &a) {
    XyzzW b = xyzzw_identity();
    if (!is_inf(a)) {
        b.x = csub_p(w_from_s(unpack<FqW>(a.x))); b.y = csub_p(w_from_s(unpack<FqW>(a.y)));
        b.zz = w_one<FqW>(); b.zzz = w_one<FqW>();
    }
    return b;
}
// bad[i] = 1 for a malformed opening: a scalar >= r, a coordinate >= q, a point that is neither (0, 0) nor on the curve
__global__ void __launch_bounds__(256) k_kzg_vm_check(uint8_t *bad, const G1Affine *cm, const Fr *zs, const Fr *ys, const G1Affine *proofs, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool ok = kz_fr_below_modulus(load_fp(zs + i)) && kz_fr_below_modulus(load_fp(ys + i)) && kz_point_ok(load_affine(cm + i)) && kz_point_ok(load_affine(proofs + i));
    bad[i] = ok ? 0 : 1;
}
// sum[i] = C_i + z_i pi_i + (-y_i) G as XYZZ on the 29-bit layer; the identity for a malformed opening, of which nothing enters the arithmetic
__global__ void __launch_bounds__(G1NTT_THREADS, 1) k_kzg_vm_front(XyzzW *sum, const uint8_t *bad, const G1Affine *cm, const Fr *zs, const Fr *ys, const G1Affine *proofs, uint32_t n) {
    extern __shared__ uint32_t g1tab[];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool ok = bad[i] == 0;
    G1Affine C, P;
    C.x = Fq::zero(); C.y = Fq::zero(); P = C;
    Fr z = Fr::zero(), y = Fr::zero();
    if (ok) { C = load_affine(cm + i); P = load_affine(proofs + i); z = load_fp(zs + i); y = load_fp(ys + i); }
    XyzzW acc = xyzzw_identity();
    if (ok) {
        G1Affine gen;                                              // the generator (1, 2)
        gen.x = Fq::one(); gen.y = add(gen.x, gen.x);
#pragma unroll 1
        for (int t = 0; t < 2; t++) {                              // ONE inlined multiplication site; the first product waits in memory, not in registers
            const XyzzW base = kz_to_w(t ? gen : P);
            const Fr k = to_canonical(t ? neg(y) : z);
            acc = g1_mul_scalar_iso(base, k, g1tab);
            if (t == 0) store_xyzzw(sum + i, acc);
        }
        const XyzzW zp = load_xyzzw(sum + i), cw = kz_to_w(C);
        g1_add_call(&acc, &zp);
        g1_add_call(&acc, &cw);
    }
    store_xyzzw(sum + i, acc);
}
// A_i = the sum as an affine point, B_i = -pi_i; (0, 0) twice for a malformed opening
__global__ void __launch_bounds__(256) k_kzg_vm_finish(G1Affine *a_out, G1Affine *b_out, const XyzzW *sum, const uint8_t *bad, const G1Affine *proofs, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine A, B;
    A.x = Fq::zero(); A.y = Fq::zero(); B = A;
    if (!bad[i]) {
        const G1Xyzz s = xyzzw_export(load_xyzzw(sum + i));
        if (!is_inf(s)) {
            const Fq zi = inv(s.zzz), iz = mul(s.zz, zi), izz = mul(iz, iz);      // 1 / ZZZ, 1 / Z, 1 / ZZ
            A.x = mul(s.x, izz); A.y = mul(s.y, zi);
        }
        const G1Affine P = load_affine(proofs + i);
        B.x = P.x; B.y = neg(P.y);                                 // (infinity stays (0, 0))
    }
    store_fp(&a_out[i].x, A.x); store_fp(&a_out[i].y, A.y);
    store_fp(&b_out[i].x, B.x); store_fp(&b_out[i].y, B.y);
}
__global__ void __launch_bounds__(256) k_kzg_vm_settle(uint8_t *verdict, const uint8_t *v, const uint8_t *bad, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) verdict[i] = bad[i] ? (uint8_t)PLK_VERDICT_MALFORMED : v[i];
}

namespace {
using namespace host;

inline Fr kz_dev(const HFr &h) { Fr f; memcpy(f.l, h.l, 32); return f; }
inline HFr kz_host(const plk_fr *p) { HFr h; memcpy(h.l, p->l, 32); return h; }
inline bool kz_fr_ok(const plk_fr *p) { return !HFr::geq_p(p->l); }
const char *const KZ_LAGRANGE_SIZE = "Lagrange-form key has a different size than the circuit's domain";     // the prover's words (prover.hip)

// Layout of the scratch of a values call: [k word | results | partials | A | B | extra]
struct ValuesPlan {
    uint32_t log_n = 0, n = 0, nb = 0, shift = 0;
    HFr z, zN;
    bool in_domain = false;
    uint32_t k = KZ_NONE;
    uint32_t *k_dev = nullptr;
    Fr *results = nullptr, *partials = nullptr, *A = nullptr, *B = nullptr, *extra = nullptr;
    KzgInv inv{};
    static size_t bytes(uint64_t n, uint64_t extra_elems) {
        const uint64_t nb = (n + KZ_BLOCK - 1) / KZ_BLOCK;
        return 256 + (size_t)(KZ_MAX + KZ_MAX * nb + 2 * n + extra_elems) * sizeof(Fr);
    }
};

// denominators, the two scans, the one inversion: after this `p.inv` serves k_kzg_sum_partial and k_kzg_div.  Waits for `st` once.
int32_t values_prepare(plk_ctx *ctx, uint32_t log_n, const HFr &z, uint64_t extra_elems, KzgScratch &ws, hipStream_t st, ValuesPlan *out) {
    ValuesPlan p;
    p.log_n = log_n; p.n = 1u << log_n; p.nb = (p.n + KZ_BLOCK - 1) / KZ_BLOCK; p.shift = MAX_LOG_N - log_n;
    p.z = z; p.zN = z.pow_u64(p.n);
    p.in_domain = p.zN == HFr::one();
    PLK_TRY(ws.reserve(ValuesPlan::bytes(p.n, extra_elems)));
    char *base = ctx->kzg_ws.as<char>();
    p.k_dev = reinterpret_cast<uint32_t *>(base);
    p.results = reinterpret_cast<Fr *>(base + 256);
    p.partials = p.results + KZ_MAX;
    p.A = p.partials + (size_t)KZ_MAX * p.nb;
    p.B = p.A + p.n;
    p.extra = p.B + p.n;
    PLK_HIP(hipMemsetAsync(p.k_dev, 0xff, 4, st));
    const Fr z_w = kz_dev(to_w(z));
    const dim3 grid((p.n + KZ_T - 1) / KZ_T);
    if (p.in_domain) hipLaunchKernelGGL(k_kzg_denoms<true>, grid, dim3(KZ_T), 0, st, p.A, p.B, ctx->tw_fwd_w, z_w, p.n, p.shift, p.k_dev);
    else hipLaunchKernelGGL(k_kzg_denoms<false>, grid, dim3(KZ_T), 0, st, p.A, p.B, ctx->tw_fwd_w, z_w, p.n, p.shift, p.k_dev);
    PLK_HIP(hipGetLastError());
    const Fr *preA = nullptr, *preB = nullptr;
    PLK_TRY(scan_pair_mult(ctx, p.A, p.A, false, true, p.B, p.B, true, true, p.n, st, &preA, &preB));
    // the grand total: behind the block prefixes (canonical), or the one block's own total (lazily reduced)
    HFr total;
    PLK_HIP(hipMemcpyAsync(total.l, ctx->poly_tmp.as<Fr>() + (p.nb > 1 ? p.nb : 0), sizeof(Fr), hipMemcpyDeviceToHost, st));
    PLK_HIP(hipMemcpyAsync(&p.k, p.k_dev, 4, hipMemcpyDeviceToHost, st));
    PLK_HIP(hipStreamSynchronize(st));
    if (HFr::geq_p(total.l)) HFr::sub_p(total.l);
    if (total.is_zero() || p.in_domain != (p.k != KZ_NONE) || (p.in_domain && p.k >= p.n)) { set_error("kzg: the denominators of the values route are inconsistent"); return PLK_ERR_HIP; }
    // what was read is 32 * T in the external form: W(1 / T) = 32 * E(1 / T) = 32 * 32 * E(1 / (32 T))
    p.inv.A = p.A; p.inv.B = p.B; p.inv.preA = preA; p.inv.preB = preB; p.inv.n = p.n;
    p.inv.s_w = kz_dev(to_w(to_w(total.inv())));
    *out = p;
    return PLK_OK;
}

// results[j] <- sum_{i != skip} (f_j[i] - y) omega^i / (omega^i - z), j < count
int32_t values_sums(plk_ctx *ctx, const ValuesPlan &p, const Fr *const *f, uint32_t count, const HFr &y, uint32_t skip, hipStream_t st) {
    KzgPolys P{};
    for (uint32_t j = 0; j < count; j++) P.f[j] = f[j];
    hipLaunchKernelGGL(k_kzg_sum_partial, dim3(p.nb, count), dim3(KZ_T), 0, st, p.partials, P, p.inv, ctx->tw_fwd_w, p.shift, kz_dev(y), skip);
    hipLaunchKernelGGL(k_kzg_sum_finish, dim3(count), dim3(KZ_T), 0, st, p.results, (const Fr *)p.partials, p.nb);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

// y_j = f_j(z): read from the arrays inside the domain, the barycentric formula f(z) = (z^N - 1) / N * sum_i f_i omega^i / (z - omega^i) outside.  Waits.
int32_t values_evaluate(plk_ctx *ctx, const ValuesPlan &p, const Fr *const *f, uint32_t count, HFr *y, hipStream_t st) {
    if (p.in_domain) {
        for (uint32_t j = 0; j < count; j++) PLK_HIP(hipMemcpyAsync(y[j].l, f[j] + p.k, sizeof(Fr), hipMemcpyDeviceToHost, st));
        PLK_HIP(hipStreamSynchronize(st));
        return PLK_OK;
    }
    PLK_TRY(values_sums(ctx, p, f, count, HFr::zero(), KZ_NONE, st));
    PLK_HIP(hipMemcpyAsync(y, p.results, count * sizeof(Fr), hipMemcpyDeviceToHost, st));
    PLK_HIP(hipStreamSynchronize(st));
    const HFr c = -((p.zN - HFr::one()) * HFr::from_u64(p.n).inv());       // the kernel sums over 1 / (omega^i - z)
    for (uint32_t j = 0; j < count; j++) y[j] = y[j] * c;
    return PLK_OK;
}

// q <- the N values of (f - y) / (x - z); y = f(z) (inside the domain the caller has checked that).  q may be f.  Waits inside the domain.
int32_t values_divide(plk_ctx *ctx, const ValuesPlan &p, const Fr *f, const HFr &y, Fr *q, hipStream_t st) {
    const dim3 grid((p.n + KZ_T - 1) / KZ_T);
    if (!p.in_domain) {
        hipLaunchKernelGGL(k_kzg_div, grid, dim3(KZ_T), 0, st, q, f, p.inv, kz_dev(y), KZ_NONE);
        PLK_HIP(hipGetLastError());
        return PLK_OK;
    }
    PLK_TRY(values_sums(ctx, p, &f, 1, y, p.k, st));               // reads f: before the division overwrites it
    hipLaunchKernelGGL(k_kzg_div, grid, dim3(KZ_T), 0, st, q, f, p.inv, kz_dev(y), p.k);
    PLK_HIP(hipGetLastError());
    HFr sum;
    PLK_HIP(hipMemcpyAsync(sum.l, p.results, sizeof(Fr), hipMemcpyDeviceToHost, st));
    PLK_HIP(hipStreamSynchronize(st));
    const HFr qk = -(sum * p.z.inv());                            // sum_{i != k} (f_i - y) omega^i / (z (z - omega^i))
    PLK_HIP(hipMemcpyAsync(q + p.k, qk.l, sizeof(Fr), hipMemcpyHostToDevice, st));
    PLK_HIP(hipStreamSynchronize(st));
    return PLK_OK;
}

int32_t kzg_common_args(const char *who, plk_ctx *ctx, const void *const *polys, uint32_t count, uint64_t n, uint32_t flags) {
    if (!ctx || !polys || count == 0 || count > KZ_MAX || n == 0 || (flags & ~(uint32_t)PLK_KZG_VALUES)) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    for (uint32_t j = 0; j < count; j++) {
        if (!polys[j]) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
        if ((uintptr_t)polys[j] & 15u) { set_error(std::string(who) + ": device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    }
    return PLK_OK;
}
}  // namespace
int32_t kzg_lagrange_key(plk_ctx *ctx, uint64_t n, uint32_t *log_n) {          // (kzg_scratch.h: kzg_multi_values.hip asks as well)
    uint32_t l = 0;
    while ((1ull << l) < n) l++;
    if (!ctx->lagrange().pts || ctx->lagrange().n != n || (1ull << l) != n || l == 0 || l > MAX_LOG_N) { set_error(KZ_LAGRANGE_SIZE); return PLK_ERR_SRS; }
    *log_n = l;
    return PLK_OK;
}
namespace {

int32_t open_coefficients(plk_ctx *ctx, const Fr *const *f, uint32_t count, uint64_t n, const HFr &z, const HFr *vp, plk_fr *evals, plk_g1_affine *proof, hipStream_t st) {
    if (!ctx->srs().pts || n > ctx->srs().n) { set_error("plk_kzg_open_dev: no key resident, or the key is shorter than the polynomials"); return PLK_ERR_SRS; }
    if (n > (1ull << MAX_LOG_N)) { set_error("plk_kzg_open_dev: more than 2^28 coefficients"); return PLK_ERR_SIZE; }
    KzgScratch ws(ctx, st);
    PLK_TRY(ws.reserve(((size_t)4 * POW_TAB + KZ_MAX + 2 * n) * sizeof(Fr)));
    Fr *tab = ctx->kzg_ws.as<Fr>(), *res = tab + 4 * POW_TAB, *t1 = res + KZ_MAX, *q = t1 + n;
    PowTable ptz, pzi;
    PLK_TRY(fill_pow_table_into(ctx, kz_dev(z), tab, &ptz, st));
    EvalArgs ea{};
    for (uint32_t j = 0; j < count; j++) { ea.poly[j] = f[j]; ea.len[j] = (uint32_t)n; ea.pt[j] = ptz; }
    ea.count = count;
    PLK_TRY(eval_batch(ctx, ea, res, st));
    PLK_HIP(hipMemcpyAsync(evals, res, count * sizeof(Fr), hipMemcpyDeviceToHost, st));
    LinCombArgs la{};
    la.count = count;
    for (uint32_t j = 0; j < count; j++) { la.s[j] = kz_dev(to_w(vp[j])); la.unit[j] = (j == 0); }
    if (!z.is_zero()) {                                            // round 5's chain: the combination times z^i, suffix sums, times z^-(k+1)
        PLK_TRY(fill_pow_table_into(ctx, kz_dev(z.inv()), tab + 2 * POW_TAB, &pzi, st));
        for (uint32_t j = 0; j < count; j++) la.p[j] = f[j];
        la.out = t1; la.n = (uint32_t)n; la.times_pow = ptz;
        PLK_TRY(lincomb(la, st));
        PLK_TRY(scan(ctx, t1, t1, (uint32_t)n, true, false, st, nullptr));
        PLK_TRY(div_finish(q, t1, pzi, (uint32_t)n, st));
    } else {                                                      // (F - c_0) / x: the combination moved down by one coefficient
        if (n > 1) {
            for (uint32_t j = 0; j < count; j++) la.p[j] = f[j] + 1;
            la.out = q; la.n = (uint32_t)(n - 1);
            PLK_TRY(lincomb(la, st));
        }
        PLK_HIP(hipMemsetAsync(q + (n - 1), 0, sizeof(Fr), st));
    }
    return msm_commit(ctx, ctx->srs(), q, n, 0, proof, st);       // waits: the evaluations have arrived as well
}

int32_t open_values(plk_ctx *ctx, const Fr *const *f, uint32_t count, uint64_t n, const HFr &z, const HFr *vp, plk_fr *evals, plk_g1_affine *proof, hipStream_t st) {
    uint32_t log_n = 0;
    PLK_TRY(kzg_lagrange_key(ctx, n, &log_n));
    KzgScratch ws(ctx, st);
    ValuesPlan p;
    PLK_TRY(values_prepare(ctx, log_n, z, n, ws, st, &p));
    HFr y[KZ_MAX], Y = HFr::zero();
    PLK_TRY(values_evaluate(ctx, p, f, count, y, st));
    for (uint32_t j = 0; j < count; j++) { memcpy(evals[j].l, y[j].l, 32); Y = Y + vp[j] * y[j]; }
    const Fr *F = f[0];
    if (count > 1) {                                               // F = sum_j v^j f_j, in values as in coefficients
        LinCombArgs la{};
        la.count = count; la.n = (uint32_t)n; la.out = p.extra;
        for (uint32_t j = 0; j < count; j++) { la.p[j] = f[j]; la.s[j] = kz_dev(to_w(vp[j])); la.unit[j] = (j == 0); }
        PLK_TRY(lincomb(la, st));
        F = p.extra;
    }
    PLK_TRY(values_divide(ctx, p, F, Y, p.extra, st));
    return msm_commit(ctx, ctx->lagrange(), p.extra, n, 0, proof, st);   // commit_using_values
}

}  // namespace
}  // namespace plk

using namespace plk;
using namespace plk::host;

extern "C" int32_t plk_poly_evaluate_values_at_dev(plk_ctx *ctx, const void *values_dev, uint32_t log_n, const plk_fr *z, plk_fr *out, void *stream) {
    if (!ctx || !values_dev || !z || !out || log_n == 0 || log_n > MAX_LOG_N || ((uintptr_t)values_dev & 15u) || !kz_fr_ok(z)) {
        set_error("plk_poly_evaluate_values_at_dev: bad argument"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    KzgScratch ws(ctx, st);
    ValuesPlan p;
    PLK_TRY(values_prepare(ctx, log_n, kz_host(z), 0, ws, st, &p));
    const Fr *f = static_cast<const Fr *>(values_dev);
    HFr y;
    PLK_TRY(values_evaluate(ctx, p, &f, 1, &y, st));
    memcpy(out->l, y.l, 32);
    return PLK_OK;
}

extern "C" int32_t plk_poly_divide_values_by_linear_dev(plk_ctx *ctx, const void *values_dev, uint32_t log_n, const plk_fr *z, const plk_fr *y, void *quotient_values_dev,
                                                        void *stream) {
    if (!ctx || !values_dev || !z || !quotient_values_dev || log_n == 0 || log_n > MAX_LOG_N || (((uintptr_t)values_dev | (uintptr_t)quotient_values_dev) & 15u) ||
        !kz_fr_ok(z) || (y && !kz_fr_ok(y))) { set_error("plk_poly_divide_values_by_linear_dev: bad argument"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    KzgScratch ws(ctx, st);
    ValuesPlan p;
    PLK_TRY(values_prepare(ctx, log_n, kz_host(z), 0, ws, st, &p));
    const Fr *f = static_cast<const Fr *>(values_dev);
    HFr yy;
    if (!y || p.in_domain) PLK_TRY(values_evaluate(ctx, p, &f, 1, &yy, st));
    if (y) {
        if (p.in_domain && yy != kz_host(y)) {
            set_error("plk_poly_divide_values_by_linear_dev: z is the point omega^" + std::to_string(p.k) + " of the domain and y differs from the value there: no polynomial quotient exists");
            return PLK_ERR_ARG;
        }
        yy = kz_host(y);
    }
    PLK_TRY(values_divide(ctx, p, f, yy, static_cast<Fr *>(quotient_values_dev), st));
    PLK_HIP(hipStreamSynchronize(st));
    return PLK_OK;
}

extern "C" int32_t plk_kzg_commit_dev(plk_ctx *ctx, const void *const *polys_dev, uint32_t count, uint64_t n, uint32_t flags, plk_g1_affine *out, void *stream) {
    if (!out) { set_error("plk_kzg_commit_dev: bad argument"); return PLK_ERR_ARG; }
    PLK_TRY(kzg_common_args("plk_kzg_commit_dev", ctx, polys_dev, count, n, flags));
    const bool values = (flags & PLK_KZG_VALUES) != 0;             // commit_using_values: against the Lagrange-form key
    if (values && (!ctx->lagrange().pts || ctx->lagrange().n != n)) { set_error(KZ_LAGRANGE_SIZE); return PLK_ERR_SRS; }
    return msm_commit_many(ctx, ctx->key[values ? KEY_LAGRANGE : KEY_MONOMIAL], polys_dev, count, n, 0, out, (hipStream_t)stream);
}

extern "C" int32_t plk_kzg_open_dev(plk_ctx *ctx, const void *const *polys_dev, uint32_t count, uint64_t n, const plk_fr *z, const plk_fr *v, uint32_t flags,
                                    plk_fr *evals, plk_g1_affine *proof, void *stream) {
    if (!z || !evals || !proof) { set_error("plk_kzg_open_dev: bad argument"); return PLK_ERR_ARG; }
    PLK_TRY(kzg_common_args("plk_kzg_open_dev", ctx, polys_dev, count, n, flags));
    if ((!v && count > 1) || !kz_fr_ok(z) || (v && !kz_fr_ok(v))) { set_error("plk_kzg_open_dev: bad argument"); return PLK_ERR_ARG; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error("plk_kzg_open_dev: a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    HFr vp[KZ_MAX];
    vp[0] = HFr::one();
    for (uint32_t j = 1; j < count; j++) vp[j] = vp[j - 1] * kz_host(v);
    const Fr *const *f = reinterpret_cast<const Fr *const *>(polys_dev);
    try {
        if (flags & PLK_KZG_VALUES) return open_values(ctx, f, count, n, kz_host(z), vp, evals, proof, st);
        return open_coefficients(ctx, f, count, n, kz_host(z), vp, evals, proof, st);
    } catch (const std::exception &e) { set_error(std::string("plk_kzg_open_dev: ") + e.what()); return PLK_ERR_HIP; }
}

extern "C" int32_t plk_kzg_verify(const plk_g1_affine *commitments, uint32_t count, const plk_fr *z, const plk_fr *evals, const plk_fr *v, const plk_g1_affine *proof,
                                  const uint8_t g2[256], int32_t *valid) {
    if (valid) *valid = 0;
    if (!commitments || !z || !evals || !proof || !g2 || !valid || count == 0 || count > KZ_MAX || (!v && count > 1)) { set_error("plk_kzg_verify: bad argument"); return PLK_ERR_ARG; }
    auto point_ok = [](const plk_g1_affine *p, HAffine *o) {
        memcpy(o, p, 64);
        return o->is_inf() || (!HFq::geq_p(p->x) && !HFq::geq_p(p->y) && on_curve(*o));
    };
    HAffine pi;
    if (!point_ok(proof, &pi)) { set_error("plk_kzg_verify: the proof is not a point of the curve"); return PLK_ERR_ARG; }
    if (!kz_fr_ok(z) || (v && !kz_fr_ok(v))) { set_error("plk_kzg_verify: a scalar is not below r"); return PLK_ERR_ARG; }
    HFr vp = HFr::one(), Y = HFr::zero();
    HJac C = HJac::inf();
    for (uint32_t j = 0; j < count; j++) {
        HAffine cj;
        if (!point_ok(commitments + j, &cj)) { set_error("plk_kzg_verify: commitment " + std::to_string(j) + " is not a point of the curve"); return PLK_ERR_ARG; }
        if (!kz_fr_ok(evals + j)) { set_error("plk_kzg_verify: a scalar is not below r"); return PLK_ERR_ARG; }
        uint64_t k[4];
        vp.to_canonical(k);
        C = jac_add(C, jac_mul(jac_from_affine(cj), k));
        Y = Y + vp * kz_host(evals + j);
        if (v) vp = vp * kz_host(v);
    }
    HAffine gen; gen.x = HFq::one(); gen.y = HFq::one() + HFq::one();
    uint64_t ky[4], kz[4];
    (-Y).to_canonical(ky);
    kz_host(z).to_canonical(kz);
    const HJac A = jac_add(jac_add(C, jac_mul(jac_from_affine(gen), ky)), jac_mul(jac_from_affine(pi), kz));
    const HAffine a = jac_to_affine(A), b = jac_to_affine(jac_neg(jac_from_affine(pi)));
    plk_g1_affine pa, pb;
    memcpy(&pa, &a, 64); memcpy(&pb, &b, 64);
    return plk_pairing_check(&pa, g2, &pb, g2 + 128, valid);
}

extern "C" int32_t plk_kzg_verify_many_dev(plk_ctx *ctx, const void *commitments_dev, const void *z_dev, const void *evals_dev, const void *proofs_dev, uint64_t n,
                                           const uint8_t g2[256], void *verdict_dev, void *stream) {
    if (!ctx || !g2 || (n && (!commitments_dev || !z_dev || !evals_dev || !proofs_dev || !verdict_dev))) { set_error("plk_kzg_verify_many_dev: null argument"); return PLK_ERR_ARG; }
    if (((uintptr_t)commitments_dev | (uintptr_t)z_dev | (uintptr_t)evals_dev | (uintptr_t)proofs_dev) & 15u) {
        set_error("plk_kzg_verify_many_dev: device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    if (n > (1ull << 28)) { set_error("plk_kzg_verify_many_dev: more than 2^28 openings"); return PLK_ERR_SIZE; }
    G2Affine q[2];
    if (!g2_from_bytes(g2, &q[0]) || !g2_from_bytes(g2 + 128, &q[1])) { set_error("plk_pairing_check: G2 point not on the twist"); return PLK_ERR_ARG; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error("plk_kzg_verify_many_dev: a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    // the call does not wait: a buffer of its own and the context's stream (on_ctx_stream, ctx.h)
    const size_t m = (size_t)(n < KZ_VM_CHUNK ? n : KZ_VM_CHUNK), pad = (m + 15) & ~(size_t)15;
    PLK_TRY(ctx->kzg_vm.reserve(m * (2 * sizeof(G1Affine) + sizeof(XyzzW)) + 2 * pad));
    char *d = ctx->kzg_vm.as<char>();
    G1Affine *a = reinterpret_cast<G1Affine *>(d), *b = a + m;
    XyzzW *tmp = reinterpret_cast<XyzzW *>(b + m);
    uint8_t *vv = reinterpret_cast<uint8_t *>(tmp + m), *bad = vv + pad;
    static_assert(sizeof(XyzzW) % 16 == 0 && sizeof(G1Affine) % 16 == 0, "the arrays behind one another stay 16-byte aligned");
    return on_ctx_stream(ctx, stream ? (hipStream_t)stream : ctx->stream, [&](hipStream_t st) -> int32_t {
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_kzg_vm_front), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO));
        for (uint64_t base = 0; base < n; base += KZ_VM_CHUNK) {
            const uint32_t cnt = (uint32_t)(n - base < KZ_VM_CHUNK ? n - base : KZ_VM_CHUNK);
            hipLaunchKernelGGL(k_kzg_vm_check, dim3((cnt + 255) / 256), dim3(256), 0, st, bad, static_cast<const G1Affine *>(commitments_dev) + base,
                               static_cast<const Fr *>(z_dev) + base, static_cast<const Fr *>(evals_dev) + base, static_cast<const G1Affine *>(proofs_dev) + base, cnt);
            hipLaunchKernelGGL(k_kzg_vm_front, dim3((cnt + G1NTT_THREADS - 1) / G1NTT_THREADS), dim3(G1NTT_THREADS), G1NTT_LDS_ISO, st, tmp, (const uint8_t *)bad,
                               static_cast<const G1Affine *>(commitments_dev) + base, static_cast<const Fr *>(z_dev) + base, static_cast<const Fr *>(evals_dev) + base,
                               static_cast<const G1Affine *>(proofs_dev) + base, cnt);
            hipLaunchKernelGGL(k_kzg_vm_finish, dim3((cnt + 255) / 256), dim3(256), 0, st, a, b, (const XyzzW *)tmp, (const uint8_t *)bad,
                               static_cast<const G1Affine *>(proofs_dev) + base, cnt);
            PLK_HIP(hipGetLastError());
            PLK_TRY(plk_pairing_check_many_dev(ctx, a, b, cnt, g2, vv, st));
            hipLaunchKernelGGL(k_kzg_vm_settle, dim3((cnt + 255) / 256), dim3(256), 0, st, static_cast<uint8_t *>(verdict_dev) + base, (const uint8_t *)vv, (const uint8_t *)bad, cnt);
            PLK_HIP(hipGetLastError());
        }
        return PLK_OK;
    });
}
