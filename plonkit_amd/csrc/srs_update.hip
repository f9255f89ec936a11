// Updating a universal key with a secret of one's own: plk_srs_update, its receipt and the receipt's check.  No counterpart in the
// reference, which can only make the tau = 42 key (src/plonk.rs:30-48) or read someone else's (src/reader.rs:67-89).
//
// The step of an updatable SRS: P'_i = s^i P_i, Q'_1 = s Q_1.  If the old key belongs to tau, the new one belongs to s tau, and it is sound
// for whoever is sure that tau OR s is unknown.  The receipt S1 = s G1, S2 = s Q_0 lets anyone check, by three pairing products and the
// key's own structure check (plk_srs_check), that the new key is the old one updated by the s committed in it — without learning s.
//
// Division of labour.  Device: the N variable-base multiplications, one lane per point, by the GLV multiplication of the G1 inverse NTT
// (g1_mul_dev.h, eight-entry effectively affine window table in LDS: one workgroup of 256 lanes per CU).  The lane forms its scalar
// s^(first + i) from the two-level power table of s with one product (k_fill_powers' formula, keycheck.hip): no vector of powers is ever
// written to memory, and the 1 MiB table is zeroed before the call returns.  The points leave as XYZZ into a scratch of the call's own
// and srs.hip's kernel brings eight at a time to affine with one inversion.  Host: s Q_1, s Q_0 on the twist (g2_host.h), s G1, and in
// the check the subgroup tests and the pairing products (pairing.cpp).
#include "ctx.h"
#include "poly.h"
#include "field29_dev.h"
#include "ec_dev.h"
#include "ec29_dev.h"
#include "g1_mul_dev.h"
#include "srs.h"
#include "pairing.h"
#include "g2_host.h"
#include "keccak.h"
#include <cerrno>
#include <cstring>
#include <sys/random.h>

namespace plk {

// out[i] = s^(first + i) * in[i], i < n, left in XYZZ (external form) for srs_to_affine.  `t` is the table of s in the 2^261 domain;
// first + n <= 2^28 (the table's reach) is the caller's to check.
__global__ void __launch_bounds__(G1NTT_THREADS, 1) srs_update_kernel(G1Xyzz *__restrict__ out, const G1Affine *__restrict__ in, PowTable t, uint64_t first, uint32_t n) {
    extern __shared__ uint32_t g1tab[];
    const uint32_t i = blockIdx.x * G1NTT_THREADS + threadIdx.x;
    if (i >= n) return;                                         // (no barrier below: a lane only touches its own column of the table)
    const G1Affine a = load_affine(in + i);
    XyzzW p = xyzzw_identity();
    if (!is_inf(a)) {
        p.x = csub_p(w_from_s(unpack<FqW>(a.x))); p.y = csub_p(w_from_s(unpack<FqW>(a.y)));
        p.zz = w_one<FqW>(); p.zzz = w_one<FqW>();
    }
    const uint32_t e = (uint32_t)(first + i);
    const FrW9 lo = unpack<FrW>(load_fp(t.lo + (e & (POW_TAB - 1)))), hi = unpack<FrW>(load_fp(t.hi + (e >> POW_SPLIT)));
    const Fr k = to_canonical(pack<FrParams>(s_from_w(mulw(lo, hi))));
    store_xyzz(out + i, xyzzw_export(g1_mul_scalar_iso8(p, k, g1tab)));
}

namespace {
using namespace host;

// device memory of one call, exact size, gone on every way out; `wipe`: zeroed on the stream first (the table of s)
struct CallBuf {
    void *p = nullptr; size_t bytes = 0; hipStream_t wipe = nullptr; bool wiped = true;
    int32_t alloc(size_t n) { PLK_HIP(hipMalloc(&p, n)); bytes = n; return PLK_OK; }
    ~CallBuf() {
        if (!p) return;
        if (!wiped) { (void)hipMemsetAsync(p, 0, bytes, wipe); (void)hipStreamSynchronize(wipe); }
        (void)hipFree(p);
    }
};
struct HostWipe {                                               // explicit_bzero of a secret on every way out
    void *p; size_t n;
    ~HostWipe() { explicit_bzero(p, n); }
};

bool fr_is_residue(const plk_fr *s) { return !HFr::geq_p(s->l); }
bool fr_is_zero(const plk_fr *s) { return (s->l[0] | s->l[1] | s->l[2] | s->l[3]) == 0; }

// 32 bytes from the OS, reduced mod r, drawn again while zero; Montgomery form
int32_t draw_secret(const char *who, HFr *out) {
    uint8_t buf[32];
    HostWipe w{buf, sizeof buf};
    for (;;) {
        for (size_t got = 0; got < 32;) {
            const ssize_t k = getrandom(buf + got, 32 - got, 0);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) { set_error(std::string(who) + ": getrandom failed"); return PLK_ERR_IO; }
            got += (size_t)k;
        }
        uint64_t c[4];
        HostWipe wc{c, sizeof c};
        memcpy(c, buf, 32);
        while (HFr::geq_p(c)) HFr::sub_p(c);                    // 2^256 / r < 6
        if (c[0] | c[1] | c[2] | c[3]) { *out = HFr::from_canonical(c); return PLK_OK; }
    }
}

// the G2 section as plk_srs_check wants it: both points on the twist (else PLK_ERR_ARG with its words), neither infinity, both of order r
int32_t parse_g2_section(const char *who, const uint8_t g2[256], G2Affine q[2], bool *sound) {
    if (!g2_from_bytes(g2, &q[0]) || !g2_from_bytes(g2 + 128, &q[1])) { set_error(std::string(who) + ": G2 point not on the twist"); return PLK_ERR_ARG; }
    *sound = !q[0].inf && !q[1].inf && g2_in_subgroup(q[0]) && g2_in_subgroup(q[1]);
    return PLK_OK;
}

// g2_new = {Q_0, s Q_1}, receipt = s G1 || s Q_0; s a non-zero residue in Montgomery form, q a sound section
void make_receipt(const HFr &s, const G2Affine q[2], const uint8_t g2_old[256], uint8_t g2_new[256], uint8_t receipt[192]) {
    uint64_t k[4];
    HostWipe w{k, sizeof k};
    s.to_canonical(k);
    HAffine g; g.x = HFq::from_u64(1); g.y = HFq::from_u64(2);
    g1_to_bytes(jac_to_affine(jac_mul(jac_from_affine(g), k)), receipt);
    g2_to_bytes(g2_to_affine(g2_mul(q[0], k)), receipt + 64);
    memcpy(g2_new, g2_old, 128);
    g2_to_bytes(g2_to_affine(g2_mul(q[1], k)), g2_new + 128);
}

HAffine neg(const HAffine &a) { HAffine r = a; if (!a.is_inf()) r.y = -a.y; return r; }
HAffine to_h(const plk_g1_affine &a) { HAffine r; memcpy(r.x.l, a.x, 32); memcpy(r.y.l, a.y, 32); return r; }

// everything of the verification that needs no device; *reason = the first rule that failed
int32_t check_receipt(const char *who, const plk_g1_affine old_p01[2], const plk_g1_affine new_p01[2], uint32_t points, const uint8_t g2_old[256],
                      const uint8_t g2_new[256], const uint8_t receipt[192], uint32_t *reason) {
    G2Affine qo[2], qn[2];
    bool so = false, sn = false;
    PLK_TRY(parse_g2_section(who, g2_old, qo, &so));
    PLK_TRY(parse_g2_section(who, g2_new, qn, &sn));
    if (!so || !sn) { *reason = PLK_UPDATE_BAD_G2; return PLK_OK; }
    if (memcmp(g2_old, g2_new, 128) != 0) { *reason = PLK_UPDATE_Q0_CHANGED; return PLK_OK; }
    const HAffine p0 = to_h(old_p01[0]);
    if (p0.is_inf() || !on_curve(p0) || memcmp(&old_p01[0], &new_p01[0], sizeof(plk_g1_affine)) != 0) { *reason = PLK_UPDATE_P0_CHANGED; return PLK_OK; }
    HAffine s1;
    if (!g1_from_bytes(receipt, &s1) || !on_curve(s1) || s1.is_inf()) { *reason = PLK_UPDATE_BAD_S1; return PLK_OK; }
    G2Affine s2;
    if (!g2_from_bytes(receipt + 64, &s2) || s2.inf || !g2_in_subgroup(s2)) { *reason = PLK_UPDATE_BAD_S2; return PLK_OK; }
    {   // e(S1, Q_0) = e(P_0, S2): S1 and S2 hold the same s
        const HAffine g1[2] = {s1, neg(p0)};
        const G2Affine g2[2] = {qo[0], s2};
        if (!pairing_product_is_one(g1, g2, 2)) { *reason = PLK_UPDATE_RECEIPT_SPLIT; return PLK_OK; }
    }
    if (points > 1) {   // e(P'_1, Q_0) = e(P_1, S2): the G1 side moved by that s
        const HAffine p1 = to_h(old_p01[1]), n1 = to_h(new_p01[1]);
        if (!on_curve(p1) || !on_curve(n1)) { *reason = PLK_UPDATE_P1_MISMATCH; return PLK_OK; }
        const HAffine g1[2] = {n1, neg(p1)};
        const G2Affine g2[2] = {qo[0], s2};
        if (!pairing_product_is_one(g1, g2, 2)) { *reason = PLK_UPDATE_P1_MISMATCH; return PLK_OK; }
    }
    {   // e(P_0, Q'_1) = e(S1, Q_1): the G2 side moved by that s
        const HAffine g1[2] = {p0, neg(s1)};
        const G2Affine g2[2] = {qn[1], qo[1]};
        if (!pairing_product_is_one(g1, g2, 2)) { *reason = PLK_UPDATE_Q1_MISMATCH; return PLK_OK; }
    }
    *reason = PLK_UPDATE_OK;
    return PLK_OK;
}

}  // namespace
}  // namespace plk

using namespace plk;

extern "C" int32_t plk_srs_update_receipt(const plk_fr *s, const uint8_t g2_old[256], uint8_t g2_new[256], uint8_t receipt[192]) {
    if (!s || !g2_old || !g2_new || !receipt) { set_error("plk_srs_update_receipt: bad argument"); return PLK_ERR_ARG; }
    if (fr_is_zero(s) || !fr_is_residue(s)) { set_error("plk_srs_update_receipt: s is zero or not a canonical residue"); return PLK_ERR_ARG; }
    G2Affine q[2];
    bool sound = false;
    PLK_TRY(parse_g2_section("plk_srs_update_receipt", g2_old, q, &sound));
    if (!sound) { set_error("plk_srs_update_receipt: a G2 point of the key is infinity or outside the subgroup"); return PLK_ERR_ARG; }
    HFr hs;
    HostWipe w{&hs, sizeof hs};
    memcpy(hs.l, s->l, 32);
    make_receipt(hs, q, g2_old, g2_new, receipt);
    return PLK_OK;
}

extern "C" int32_t plk_srs_update_check_receipt(const plk_g1_affine old_p01[2], const plk_g1_affine new_p01[2], uint32_t points, const uint8_t g2_old[256],
                                                const uint8_t g2_new[256], const uint8_t receipt[192], int32_t *valid, uint32_t *reason) {
    if (valid) *valid = 0;
    if (reason) *reason = PLK_UPDATE_OK;
    if (!old_p01 || !new_p01 || points == 0 || !g2_old || !g2_new || !receipt || !valid) { set_error("plk_srs_update_check_receipt: bad argument"); return PLK_ERR_ARG; }
    uint32_t why = PLK_UPDATE_OK;
    PLK_TRY(check_receipt("plk_srs_update_check_receipt", old_p01, new_p01, points, g2_old, g2_new, receipt, &why));
    if (reason) *reason = why;
    *valid = why == PLK_UPDATE_OK ? 1 : 0;
    return PLK_OK;
}

extern "C" int32_t plk_srs_update_verify(plk_ctx *ctx, const plk_g1_affine old_p01[2], const uint8_t g2_old[256], const uint8_t g2_new[256],
                                         const uint8_t receipt[192], const uint8_t seed[32], int32_t *valid, uint32_t *reason) {
    if (valid) *valid = 0;
    if (reason) *reason = PLK_UPDATE_OK;
    if (!ctx || !old_p01 || !g2_old || !g2_new || !receipt || !valid) { set_error("plk_srs_update_verify: bad argument"); return PLK_ERR_ARG; }
    if (!ctx->srs().pts || ctx->srs().n == 0) { set_error("plk_srs_update_verify: no key resident"); return PLK_ERR_SRS; }
    if (ctx->shard_first != 0) { set_error("plk_srs_update_verify: this context holds a slice of the key (first index " + std::to_string(ctx->shard_first) + "): the check needs the whole prefix"); return PLK_ERR_ARG; }
    const uint32_t points = ctx->srs().n > 1 ? 2 : 1;
    plk_g1_affine new_p01[2] = {};
    PLK_TRY(plk_srs_download(ctx, 0, points, new_p01));
    uint32_t why = PLK_UPDATE_OK;
    PLK_TRY(check_receipt("plk_srs_update_verify", old_p01, new_p01, points, g2_old, g2_new, receipt, &why));
    if (why == PLK_UPDATE_OK) {
        int32_t key_ok = 0;
        PLK_TRY(plk_srs_check(ctx, g2_new, seed, 0, &key_ok, nullptr));
        if (!key_ok) why = PLK_UPDATE_KEY_STRUCTURE;
    }
    if (reason) *reason = why;
    *valid = why == PLK_UPDATE_OK ? 1 : 0;
    return PLK_OK;
}

extern "C" int32_t plk_srs_update(plk_ctx *ctx, const plk_fr *s, uint64_t first, const uint8_t g2_old[256], uint8_t g2_new[256], uint8_t receipt[192]) {
    if (!ctx || !g2_old || !g2_new || !receipt) { set_error("plk_srs_update: bad argument"); return PLK_ERR_ARG; }
    if (!ctx->srs().pts || ctx->srs().n == 0) { set_error("plk_srs_update: no key resident"); return PLK_ERR_SRS; }
    const uint64_t n = ctx->srs().n;
    if (n > (1ull << MAX_LOG_N) || first > (1ull << MAX_LOG_N) - n) { set_error("plk_srs_update: the highest index, first + size, exceeds 2^28 (the reach of the table of powers of s)"); return PLK_ERR_SIZE; }
    if (s && (fr_is_zero(s) || !fr_is_residue(s))) { set_error("plk_srs_update: s is zero or not a canonical residue"); return PLK_ERR_ARG; }
    G2Affine q[2];
    bool sound = false;
    PLK_TRY(parse_g2_section("plk_srs_update", g2_old, q, &sound));
    if (!sound) { set_error("plk_srs_update: a G2 point of the key is infinity or outside the subgroup"); return PLK_ERR_ARG; }
    // refused before anything is computed; the guard itself runs when the new key is installed (on a borrower it returns the loan,
    // which a failed call must leave as it was)
    if (ctx->srs().borrowers.load() > 0) return srs_replace_guard(ctx, "plk_srs_update");
    if (ctx->msm_enq != ctx->msm_fin) { set_error("plk_srs_update: a commitment is still in flight on this context"); return PLK_ERR_ARG; }

    HFr hs;
    HostWipe wipe_s{&hs, sizeof hs};
    if (s) memcpy(hs.l, s->l, 32);
    else PLK_TRY(draw_secret("plk_srs_update", &hs));
    uint8_t g2_out[256], receipt_out[192];                      // the caller's buffers are written on success only
    make_receipt(hs, q, g2_old, g2_out, receipt_out);

    PLK_HIP(hipSetDevice(ctx->device));
    PLK_HIP(hipStreamSynchronize(ctx->stream));                 // earlier work on the key
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(srs_update_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO8));
        attr_set = true;
    }
    ctx->update_ms_valid = false;
    StageTimer<2> timed;                                        // plk_set_kernel_timing: a bracket around the device work
    PLK_TRY(timed.start(ctx));
    PLK_TRY(timed.mark(0, ctx->stream));
    DevBuf fresh;                                               // the new key: the context's own once the last chunk is done
    struct Drop { DevBuf &b; ~Drop() { b.release(); } } drop{fresh};
    PLK_TRY(fresh.reserve(n * sizeof(G1Affine)));
    const uint64_t chunk = n < SRS_CHUNK ? n : SRS_CHUNK;
    CallBuf scratch, table;
    PLK_TRY(scratch.alloc(chunk * sizeof(G1Xyzz)));
    PLK_TRY(table.alloc((size_t)2 * POW_TAB * sizeof(Fr)));
    table.wipe = ctx->stream; table.wiped = false;
    PowTable pt;
    {
        Fr base;
        HostWipe wipe_b{&base, sizeof base};
        memcpy(base.l, hs.l, 32);
        PLK_TRY(fill_pow_table_into(ctx, base, reinterpret_cast<Fr *>(table.p), &pt, ctx->stream));
    }
    const G1Affine *old = reinterpret_cast<const G1Affine *>(ctx->srs().pts);
    G1Xyzz *tmp = reinterpret_cast<G1Xyzz *>(scratch.p);
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint64_t len = n - off < chunk ? n - off : chunk;
        hipLaunchKernelGGL(srs_update_kernel, dim3((uint32_t)((len + G1NTT_THREADS - 1) / G1NTT_THREADS)), dim3(G1NTT_THREADS), G1NTT_LDS_ISO8, ctx->stream,
                           tmp, old + off, pt, first + off, (uint32_t)len);
        PLK_HIP(hipGetLastError());
        PLK_TRY(srs_to_affine(fresh.as<G1Affine>() + off, tmp, len, ctx->stream));
    }
    PLK_TRY(timed.mark(1, ctx->stream));
    PLK_HIP(hipStreamSynchronize(ctx->stream));
    if (timed.on) { PLK_TRY(timed.elapsed(0, 1, &ctx->update_ms)); ctx->update_ms_valid = true; }

    PLK_TRY(srs_replace_guard(ctx, "plk_srs_update"));
    key_install_owned(ctx, KEY_MONOMIAL, fresh, n);             // (`fresh` now holds the old key, if the context owned it: released on the way out)
    key_clear(ctx, KEY_LAGRANGE);                               // the old Lagrange-form key no longer belongs
    memcpy(g2_new, g2_out, 256);
    memcpy(receipt, receipt_out, 192);
    return PLK_OK;
}

extern "C" int32_t plk_srs_update_last_ms(plk_ctx *ctx, float *out_ms) {
    if (!ctx || !out_ms) { set_error("plk_srs_update_last_ms: bad argument"); return PLK_ERR_ARG; }
    if (!ctx->update_ms_valid) { set_error("plk_srs_update_last_ms: no timed plk_srs_update on this context (plk_set_kernel_timing)"); return PLK_ERR_ARG; }
    *out_ms = ctx->update_ms;
    return PLK_OK;
}
