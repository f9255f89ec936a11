// Structure checks of the resident key(s): plk_srs_check (powers of tau against the G2 section; plk_srs_check_points_dev: the same
// verdict on points in device memory that are not installed) and plk_srs_lagrange_check (the Lagrange-form key against the monomial one).  No counterpart in the reference: bellman's Crs::read (src/reader.rs:67-89) checks
// that every point is on the curve and nothing else.  Statement, error bound and status codes: include/plonkit_amd.h.
//
// Division of labour.  Device: the vector rho^i (one kernel over the two-level power table the prover's rounds use: PowTable,
// fill_pow_table_into — one product per element, no serial chain), the commitments T = sum rho^i P_i through the existing pipeline
// (plk_msm_g1_dev: it cuts vectors above 2^24 terms itself; a sub-range of the bisection is base_offset = lo with the same vector
// from index 0) and, for the Lagrange form, one inverse transform of that vector (plk_ntt_dev).  Host: keccak, the two [r]Q = O
// subgroup checks on the twist, a handful of G1 operations on 64-byte points and the pairing product (pairing.cpp).
// The vector lives in the prover's workspace (ctx->prove_ws, behind the 1 MiB power table) for the duration of a call; a call that
// had to grow the workspace frees it before it returns, so nothing stays allocated for the life of the context.
#include "ctx.h"
#include "poly.h"
#include "msm.h"
#include "ec_dev.h"
#include "field29_dev.h"
#include "pairing.h"
#include "g2_host.h"
#include "keccak.h"
#include <cerrno>
#include <cstring>
#include <sys/random.h>

namespace plk {

constexpr uint64_t KEYCHECK_NONE = ~0ull;

// out_i = rho^i, i < n, in the library's external form (Montgomery, R = 2^256).  `t` is rho's table in the 2^261 domain: W(lo) * W(hi) * 2^-261
// = W(lo * hi), and s_from_w brings that to x * 2^256, canonical.  A wave reads 64 consecutive lo entries and one hi entry.
__global__ void __launch_bounds__(256) k_fill_powers(Fr *__restrict__ out, PowTable t, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const FrW9 lo = unpack<FrW>(load_fp(t.lo + (i & (POW_TAB - 1)))), hi = unpack<FrW>(load_fp(t.hi + (i >> POW_SPLIT)));
    store_fp(out + i, pack<FrParams>(s_from_w(mulw(lo, hi))));
}

namespace {
using namespace host;

// rho = keccak256(tag || seed) mod r, hashed again while it is zero; seed == nullptr: 32 bytes from the OS
int32_t derive_rho(const char *tag, const uint8_t *seed, HFr *rho) {
    uint8_t buf[64], h[32];
    const size_t tl = strlen(tag);                              // (both tags are shorter than 32 bytes)
    memcpy(buf, tag, tl);
    if (seed) memcpy(buf + tl, seed, 32);
    else {
        for (size_t got = 0; got < 32;) {
            const ssize_t k = getrandom(buf + tl + got, 32 - got, 0);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) { set_error(std::string(tag) + ": getrandom failed"); return PLK_ERR_IO; }
            got += (size_t)k;
        }
    }
    keccak256(buf, tl + 32, h);
    for (;;) {
        uint64_t c[4] = {0, 0, 0, 0};
        for (int i = 0; i < 4; i++) for (int b = 0; b < 8; b++) c[i] |= (uint64_t)h[31 - (8 * i + b)] << (8 * b);
        while (HFr::geq_p(c)) HFr::sub_p(c);                    // 2^256 / r < 6
        if (c[0] | c[1] | c[2] | c[3]) { *rho = HFr::from_canonical(c); return PLK_OK; }
        uint8_t again[32];
        keccak256(h, 32, again);
        memcpy(h, again, 32);
    }
}

// (the twist arithmetic of the two [r]Q = O checks: g2_host.h)

// Where the n points under check live: the resident monomial key (plk_srs_check: commitments through msm_commit and the key's fixed-base
// table, points by plk_srs_download) or n points in device memory that are no key (plk_srs_check_points_dev: commitments through the
// caller-supplied-bases path, msm_bases_commit, which builds no table and touches nothing resident).  Everything else is shared.
struct KeyPoints {
    plk_ctx *ctx;
    const G1Affine *dev;                                        // nullptr: the resident key
    uint64_t n;
    // sum_{i<m} pows[i] * P_{lo+i}
    int32_t commit(const Fr *pows, uint64_t lo, uint64_t m, HAffine *T) const {
        if (!dev) {
            plk_g1_affine t;
            PLK_TRY(msm_commit(ctx, ctx->srs(), pows, m, lo, &t, nullptr));
            memcpy(T, &t, 64);
            return PLK_OK;
        }
        HJac j; uint64_t bad;
        PLK_TRY(msm_bases_commit(ctx, dev + lo, &pows, 1, m, false, &bad, ctx->stream, &j));
        *T = jac_to_affine(j);
        return PLK_OK;
    }
    int32_t fetch(uint64_t i, HAffine *p) const {
        if (!dev) {
            plk_g1_affine a;
            PLK_TRY(plk_srs_download(ctx, i, 1, &a));
            memcpy(p, &a, 64);
            return PLK_OK;
        }
        PLK_HIP(hipMemcpyAsync(p, dev + i, 64, hipMemcpyDeviceToHost, ctx->stream));
        PLK_HIP(hipStreamSynchronize(ctx->stream));
        return PLK_OK;
    }
};

// The workspace only grows, and a proof on a small domain never asks for what the check of a large key does (2 GiB at 2^26 points): a call
// that had to grow it gives it back on every way out (all commitments of the call have finished by then: they are synchronous).
struct WorkspaceLoan {
    plk_ctx *ctx; bool grew = false;
    ~WorkspaceLoan() { if (grew) { (void)hipStreamSynchronize(ctx->stream); ctx->prove_ws.release(); } }
};

// the table of rho and rho^i, i < n, in the prover's workspace
int32_t fill_powers(plk_ctx *ctx, const HFr &rho, uint64_t n, Fr **pows, WorkspaceLoan *loan) {
    PLK_HIP(hipStreamSynchronize(ctx->stream));                 // earlier users of the workspace
    const size_t bytes = ((size_t)2 * POW_TAB + n) * sizeof(Fr);
    loan->grew = bytes > ctx->prove_ws.cap;
    PLK_TRY(ctx->prove_ws.reserve(bytes));
    ctx->trace.valid = false;                                   // (plk_prove_trace's vectors lived there)
    Fr *tab = ctx->prove_ws.as<Fr>(), base;
    memcpy(base.l, rho.l, 32);
    PowTable pt;
    PLK_TRY(fill_pow_table_into(ctx, base, tab, &pt, ctx->stream));
    *pows = tab + 2 * POW_TAB;
    hipLaunchKernelGGL(k_fill_powers, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, *pows, pt, (uint32_t)n);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

// the links between the m points from index lo, by one commitment: T = sum_{i<m} rho^i P_{lo+i}, A = T - P_lo,
// B = rho (T - rho^(m-1) P_{lo+m-1}); they hold (up to the bound of the header) iff e(A, Q_0) e(-B, Q_1) = 1
int32_t links_hold(const KeyPoints &pts, const Fr *pows, uint64_t lo, uint64_t m, const HFr &rho, const G2Affine q[2], bool *ok) {
    *ok = true;
    if (m < 2) return PLK_OK;
    HAffine T, first, last;
    PLK_TRY(pts.commit(pows, lo, m, &T));
    PLK_TRY(pts.fetch(lo, &first));
    PLK_TRY(pts.fetch(lo + m - 1, &last));
    uint64_t top[4], r1[4];
    rho.pow_u64(m - 1).to_canonical(top);
    rho.to_canonical(r1);
    const HJac Tj = jac_from_affine(T);
    const HJac A = jac_add(Tj, jac_neg(jac_from_affine(first)));
    const HJac B = jac_mul(jac_add(Tj, jac_neg(jac_mul(jac_from_affine(last), top))), r1);
    const HAffine g1[2] = {jac_to_affine(A), jac_to_affine(jac_neg(B))};
    *ok = pairing_product_is_one(g1, q, 2);
    return PLK_OK;
}

// plk_srs_check and plk_srs_check_points_dev after their own argument checks: the verdict on pts.n >= 1 points (statement: include/plonkit_amd.h)
int32_t check_powers(const char *who, const KeyPoints &pts, const G2Affine q[2], const uint8_t *seed, uint32_t flags, int32_t *valid, uint64_t *bad_out) {
    plk_ctx *ctx = pts.ctx;
    const uint64_t n = pts.n;
    if (n > (1ull << MAX_LOG_N)) { set_error(std::string(who) + ": more than 2^28 points"); return PLK_ERR_SIZE; }
    HFr rho;
    PLK_TRY(derive_rho("plk_srs_check", seed, &rho));
    PLK_HIP(hipSetDevice(ctx->device));
    HAffine p0;
    PLK_TRY(pts.fetch(0, &p0));
    if (p0.is_inf()) { if (bad_out) *bad_out = 0; return PLK_OK; }          // (an all-infinity key would pass the pairing identity)
    if (q[0].inf || q[1].inf || !g2_in_subgroup(q[0]) || !g2_in_subgroup(q[1])) return PLK_OK;
    if (n == 1) { *valid = 1; return PLK_OK; }
    Fr *pows = nullptr;
    WorkspaceLoan loan{ctx};
    PLK_TRY(fill_powers(ctx, rho, n, &pows, &loan));
    bool ok = false;
    PLK_TRY(links_hold(pts, pows, 0, n, rho, q, &ok));
    if (ok) { *valid = 1; return PLK_OK; }
    if (!(flags & PLK_KEY_LOCATE)) return PLK_OK;
    // every link below lo holds, one of [lo, hi) does not: the points [lo, mid] decide which half
    uint64_t lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        PLK_TRY(links_hold(pts, pows, lo, mid - lo + 1, rho, q, &ok));
        if (ok) lo = mid; else hi = mid;
    }
    if (bad_out) *bad_out = lo;
    return PLK_OK;
}

}  // namespace
}  // namespace plk

using namespace plk;

extern "C" int32_t plk_srs_check(plk_ctx *ctx, const uint8_t g2[256], const uint8_t seed[32], uint32_t flags, int32_t *valid, uint64_t *bad_out) {
    if (bad_out) *bad_out = KEYCHECK_NONE;
    if (valid) *valid = 0;
    if (!ctx || !g2 || !valid || (flags & ~PLK_KEY_LOCATE)) { set_error("plk_srs_check: bad argument"); return PLK_ERR_ARG; }
    G2Affine q[2];
    if (!g2_from_bytes(g2, &q[0]) || !g2_from_bytes(g2 + 128, &q[1])) { set_error("plk_srs_check: G2 point not on the twist"); return PLK_ERR_ARG; }
    if (!ctx->srs().pts || ctx->srs().n == 0) { set_error("plk_srs_check: no key resident"); return PLK_ERR_SRS; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error("plk_srs_check: a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    return check_powers("plk_srs_check", KeyPoints{ctx, nullptr, ctx->srs().n}, q, seed, flags, valid, bad_out);
}

// the same verdict on n points in device memory that are not installed (and need not be): nothing resident is read or changed
extern "C" int32_t plk_srs_check_points_dev(plk_ctx *ctx, const void *points_dev, uint64_t n, const uint8_t g2[256], const uint8_t seed[32], uint32_t flags,
                                            int32_t *valid, uint64_t *bad_out, void *stream) {
    if (bad_out) *bad_out = KEYCHECK_NONE;
    if (valid) *valid = 0;
    if (!ctx || !g2 || !valid || (flags & ~PLK_KEY_LOCATE) || (n && !points_dev) || ((uintptr_t)points_dev & 15u)) { set_error("plk_srs_check_points_dev: bad argument"); return PLK_ERR_ARG; }
    G2Affine q[2];
    if (!g2_from_bytes(g2, &q[0]) || !g2_from_bytes(g2 + 128, &q[1])) { set_error("plk_srs_check_points_dev: G2 point not on the twist"); return PLK_ERR_ARG; }
    if (n == 0) { set_error("plk_srs_check_points_dev: no points"); return PLK_ERR_SRS; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error("plk_srs_check_points_dev: a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    if (stream && (hipStream_t)stream != ctx->stream) PLK_HIP(hipStreamSynchronize((hipStream_t)stream));   // the points are complete; the call itself runs on the context's stream
    BasesScratchLoan scratch(ctx);                              // (one loan for the whole bisection)
    return check_powers("plk_srs_check_points_dev", KeyPoints{ctx, static_cast<const G1Affine *>(points_dev), n}, q, seed, flags, valid, bad_out);
}

extern "C" int32_t plk_srs_lagrange_check(plk_ctx *ctx, const uint8_t seed[32], int32_t *valid) {
    if (valid) *valid = 0;
    if (!ctx || !valid) { set_error("plk_srs_lagrange_check: bad argument"); return PLK_ERR_ARG; }
    if (ctx->shard_first != 0) { set_error("plk_srs_lagrange_check: this context holds a slice of the key (first index " + std::to_string(ctx->shard_first) + "): tying the two forms needs the whole prefix"); return PLK_ERR_ARG; }
    if (ctx->msm_enq != ctx->msm_fin) { set_error("plk_srs_lagrange_check: a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    if (!ctx->lagrange().pts || ctx->lagrange().n == 0) { set_error("plk_srs_lagrange_check: no Lagrange-form key resident"); return PLK_ERR_SRS; }
    const uint64_t N = ctx->lagrange().n;
    if (!ctx->srs().pts || ctx->srs().n < N) { set_error("plk_srs_lagrange_check: the monomial key is missing or shorter than the Lagrange-form key"); return PLK_ERR_SRS; }
    uint32_t log_n = 0;
    while ((1ull << log_n) < N) log_n++;
    if ((1ull << log_n) != N || log_n > MAX_LOG_N) { set_error("plk_srs_lagrange_check: the Lagrange-form key's size is not a power of two"); return PLK_ERR_SIZE; }
    HFr rho;
    PLK_TRY(derive_rho("plk_srs_lagrange_check", seed, &rho));
    PLK_HIP(hipSetDevice(ctx->device));
    Fr *pows = nullptr;
    WorkspaceLoan loan{ctx};
    PLK_TRY(fill_powers(ctx, rho, N, &pows, &loan));
    plk_g1_affine by_values, by_coeffs;
    PLK_TRY(msm_commit(ctx, ctx->lagrange(), pows, N, 0, &by_values, nullptr));
    if (log_n) PLK_TRY(plk_ntt_dev(ctx, pows, log_n, 1, nullptr, nullptr));
    PLK_TRY(msm_commit(ctx, ctx->srs(), pows, N, 0, &by_coeffs, nullptr));
    *valid = memcmp(&by_values, &by_coeffs, sizeof by_values) == 0 ? 1 : 0;
    return PLK_OK;
}
