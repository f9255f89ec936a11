// Key files on the GPU: Crs::read / Crs::write (src/reader.rs:67-89; src/bin/main.rs:341,379) without a host pass over the points.
// The file stores a G1 point as x ‖ y, 32 big-endian canonical bytes each, infinity as 0x40 00..00; the resident key
// is x ‖ y in Montgomery form with infinity = all zero.  Decode = byte swap, range check, two products by R^2 and the curve equation
// (five Montgomery products per point); encode = two products by 1 and a byte swap.  One lane owns one point: four dwordx4 loads and
// four dwordx4 stores with a 64-byte lane stride, every byte of every line used.  Against the host-to-device copy of the same chunk
// the kernels are noise (profiles/key_io_ab.txt), so there is no LDS staging.
//
// A point is refused exactly when the host pair g1_from_bytes + on_curve (hostapi.cpp, hostmath.h) refuses it — pairing_ce's
// G1Uncompressed::into_affine.  The verdict of a whole buffer is the LOWEST refused index (atomicMin on one 64-bit word), so it does
// not depend on the launch geometry or on how plk_srs_load_key cuts the file into chunks.
#include "ctx.h"
#include "ec_dev.h"
#include <cstring>

namespace plk {

int32_t g1_intt_dev(plk_ctx *ctx, const G1Affine *in, uint32_t log_n, G1Affine *out, hipStream_t st);   // g1ntt.hip

constexpr uint64_t KEY_CHUNK_POINTS = 1ull << 20;          // points per staging buffer: 64 MiB of file bytes, two buffers
constexpr uint64_t KEY_NONE = ~0ull;                       // the verdict word while no point has been refused

// 32 big-endian bytes (as two dwordx4) -> canonical little-endian limbs; false if the value is >= q
__device__ __forceinline__ bool be_to_limbs(const u32x4 &a, const u32x4 &b, Fq *out) {
    out->l[7] = __builtin_bswap32(a.x); out->l[6] = __builtin_bswap32(a.y); out->l[5] = __builtin_bswap32(a.z); out->l[4] = __builtin_bswap32(a.w);
    out->l[3] = __builtin_bswap32(b.x); out->l[2] = __builtin_bswap32(b.y); out->l[1] = __builtin_bswap32(b.z); out->l[0] = __builtin_bswap32(b.w);
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)out->l[i] - FqParams::P[i] - br; br = (d >> 32) & 1; }
    return br != 0;                                         // a borrow out of the top limb: value < q
}
__device__ __forceinline__ void limbs_to_be(const Fq &v, u32x4 *a, u32x4 *b) {
    *a = u32x4{__builtin_bswap32(v.l[7]), __builtin_bswap32(v.l[6]), __builtin_bswap32(v.l[5]), __builtin_bswap32(v.l[4])};
    *b = u32x4{__builtin_bswap32(v.l[3]), __builtin_bswap32(v.l[2]), __builtin_bswap32(v.l[1]), __builtin_bswap32(v.l[0])};
}

// bytes: `n` points of the file, 16-byte aligned.  Point i has the global index base + i (what a refusal reports) and is stored to
// out[base + i - keep_first] if that lies in [0, keep_count): every point is checked, a slice is kept.
__global__ void __launch_bounds__(256) g1_decode_kernel(const u32x4 *__restrict__ bytes, uint64_t n, uint64_t base, G1Affine *__restrict__ out,
                                                        uint64_t keep_first, uint64_t keep_count, unsigned long long *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32x4 w0 = bytes[4 * i], w1 = bytes[4 * i + 1], w2 = bytes[4 * i + 2], w3 = bytes[4 * i + 3];
    const uint32_t b0 = w0.x & 0xffu;                       // byte 0 of the encoding: the flag bits
    G1Affine p; p.x = Fq::zero(); p.y = Fq::zero();
    bool ok;
    if (b0 & 0x40u) {                                       // infinity: exactly 0x40 followed by 63 zero bytes
        const uint32_t rest = (w0.x ^ 0x40u) | w0.y | w0.z | w0.w | w1.x | w1.y | w1.z | w1.w | w2.x | w2.y | w2.z | w2.w | w3.x | w3.y | w3.z | w3.w;
        ok = rest == 0;
    } else if (b0 & 0x80u) {                                // compression flag on an uncompressed encoding
        ok = false;
    } else {
        Fq x, y;
        const bool xin = be_to_limbs(w0, w1, &x), yin = be_to_limbs(w2, w3, &y);
        ok = xin && yin && !(x.is_zero() && y.is_zero());   // (0, 0) without the flag is an ordinary point, and not on the curve
        if (ok) {
            p.x = from_canonical(x); p.y = from_canonical(y);
            ok = g1_on_curve(p);                            // y^2 = x^3 + 3 (ec_dev.h)
            if (!ok) { p.x = Fq::zero(); p.y = Fq::zero(); }
        }
    }
    const uint64_t g = base + i;
    if (!ok) atomicMin(bad, (unsigned long long)g);
    if (g >= keep_first && g - keep_first < keep_count) {
        store_fp(&out[g - keep_first].x, p.x);
        store_fp(&out[g - keep_first].y, p.y);
    }
}

__global__ void __launch_bounds__(256) g1_encode_kernel(const G1Affine *__restrict__ pts, uint64_t n, u32x4 *__restrict__ bytes) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fq x = load_fp(&pts[i].x), y = load_fp(&pts[i].y);
    u32x4 w0, w1, w2, w3;
    if (x.is_zero() && y.is_zero()) {
        w0 = u32x4{0x40u, 0, 0, 0}; w1 = w2 = w3 = u32x4{0, 0, 0, 0};
    } else {
        limbs_to_be(to_canonical(x), &w0, &w1);
        limbs_to_be(to_canonical(y), &w2, &w3);
    }
    bytes[4 * i] = w0; bytes[4 * i + 1] = w1; bytes[4 * i + 2] = w2; bytes[4 * i + 3] = w3;
}

static inline void launch_decode(const void *bytes, uint64_t n, uint64_t base, void *out, uint64_t keep_first, uint64_t keep_count, void *bad, hipStream_t st) {
    hipLaunchKernelGGL(g1_decode_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, (const u32x4 *)bytes, n, base, (G1Affine *)out,
                       keep_first, keep_count, (unsigned long long *)bad);
}
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// two streams' worth of events around the double buffer; destroyed whatever way the call ends
struct KeyPipe {
    hipStream_t copy = nullptr;
    hipEvent_t filled[2] = {nullptr, nullptr}, drained[2] = {nullptr, nullptr};
    int32_t open() {
        PLK_HIP(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) {
            PLK_HIP(hipEventCreateWithFlags(&filled[k], hipEventDisableTiming));
            PLK_HIP(hipEventCreateWithFlags(&drained[k], hipEventDisableTiming));
        }
        return PLK_OK;
    }
    ~KeyPipe() {
        if (copy) { (void)hipStreamSynchronize(copy); (void)hipStreamDestroy(copy); }
        for (int k = 0; k < 2; k++) { if (filled[k]) (void)hipEventDestroy(filled[k]); if (drained[k]) (void)hipEventDestroy(drained[k]); }
    }
};

// staging of both directions: two chunk buffers and the verdict word, in the context's staging arena
static int32_t key_stage(plk_ctx *ctx, uint64_t n, uint64_t *chunk, char **buf0, char **buf1, unsigned long long **bad) {
    *chunk = n < KEY_CHUNK_POINTS ? (n ? n : 1) : KEY_CHUNK_POINTS;
    const size_t cb = (size_t)*chunk * 64;
    PLK_TRY(ctx->stage.reserve(2 * cb + 16));
    *buf0 = ctx->stage.as<char>(); *buf1 = *buf0 + cb;
    *bad = reinterpret_cast<unsigned long long *>(*buf0 + 2 * cb);
    return PLK_OK;
}

}  // namespace plk

using namespace plk;

extern "C" uint64_t plk_key_chunk_points(void) { return KEY_CHUNK_POINTS; }

extern "C" int32_t plk_g1_decode_dev(plk_ctx *ctx, const void *bytes_dev, uint64_t n, void *points_dev, uint64_t *bad_out, void *stream) {
    if (bad_out) *bad_out = KEY_NONE;
    if (!ctx || (n && (!bytes_dev || !points_dev)) || !aligned16(bytes_dev) || !aligned16(points_dev)) { set_error("plk_g1_decode_dev: bad argument"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    PLK_TRY(ctx->key_bad.reserve(16));
    unsigned long long bad = KEY_NONE;
    PLK_HIP(hipMemsetAsync(ctx->key_bad.p, 0xff, 8, s));
    launch_decode(bytes_dev, n, 0, points_dev, 0, n, ctx->key_bad.p, s);
    PLK_HIP(hipGetLastError());
    PLK_HIP(hipMemcpyAsync(&bad, ctx->key_bad.p, 8, hipMemcpyDeviceToHost, s));
    PLK_HIP(hipStreamSynchronize(s));                        // the verdict is this call's return value
    if (bad_out) *bad_out = bad;
    if (bad != KEY_NONE) { set_error("read key err: point not on curve"); return PLK_ERR_FORMAT; }
    return PLK_OK;
}

extern "C" int32_t plk_g1_encode_dev(plk_ctx *ctx, const void *points_dev, uint64_t n, void *bytes_dev, void *stream) {
    if (!ctx || (n && (!bytes_dev || !points_dev)) || !aligned16(bytes_dev) || !aligned16(points_dev)) { set_error("plk_g1_encode_dev: bad argument"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    hipLaunchKernelGGL(g1_encode_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (const G1Affine *)points_dev, n, (u32x4 *)bytes_dev);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

extern "C" int32_t plk_srs_load_key(plk_ctx *ctx, const uint8_t *data, uint64_t len, uint64_t first, uint64_t count, uint32_t flags,
                                    uint64_t *n_out, uint8_t g2_out[256], uint64_t *bad_out) {
    if (bad_out) *bad_out = KEY_NONE;
    if (!ctx || !data || !n_out || (flags & ~PLK_KEY_LAGRANGE)) { set_error("plk_srs_load_key: bad argument"); return PLK_ERR_ARG; }
    const bool lagrange = (flags & PLK_KEY_LAGRANGE) != 0;
    PLK_TRY(plk_key_parse(data, len, nullptr, 0, n_out, g2_out));            // the container: same checks, codes and words
    const uint64_t n = *n_out;
    if (first > n || count > n - first) { set_error("plk_srs_load_key: slice outside the key"); return PLK_ERR_ARG; }
    const uint64_t kept = count ? count : n - first;
    if (kept == 0) { set_error("plk_srs_load_key: nothing to keep resident"); return PLK_ERR_ARG; }
    // a lender is refused before any work; a borrower's loan is only dropped once the new key is complete (the guard below)
    const KeyForm which = lagrange ? KEY_LAGRANGE : KEY_MONOMIAL;
    if (ctx->key[which].borrowers.load() > 0) return srs_replace_guard(ctx, "plk_srs_load_key", which);
    PLK_HIP(hipSetDevice(ctx->device));
    DevBuf fresh;                                                             // the old key stays what it is until every chunk has passed
    struct Drop { DevBuf &b; ~Drop() { b.release(); } } drop{fresh};
    PLK_TRY(fresh.reserve(kept * sizeof(G1Affine)));
    uint64_t chunk; char *buf[2]; unsigned long long *bad_dev;
    PLK_TRY(key_stage(ctx, n, &chunk, &buf[0], &buf[1], &bad_dev));
    KeyPipe pipe;
    PLK_TRY(pipe.open());
    PLK_HIP(hipStreamSynchronize(ctx->stream));                               // earlier users of the staging arena
    PLK_HIP(hipMemsetAsync(bad_dev, 0xff, 8, ctx->stream));
    // copy k + 1 (copy stream; from pageable memory the call itself waits for it) runs beside kernel k (the context's stream)
    uint32_t k = 0;
    for (uint64_t off = 0; off < n; off += chunk, k++) {
        const uint64_t m = n - off < chunk ? n - off : chunk;
        const int b = k & 1;
        if (k >= 2) PLK_HIP(hipStreamWaitEvent(pipe.copy, pipe.drained[b], 0));
        PLK_HIP(hipMemcpyAsync(buf[b], data + 8 + 64 * off, 64 * m, hipMemcpyHostToDevice, pipe.copy));
        PLK_HIP(hipEventRecord(pipe.filled[b], pipe.copy));
        PLK_HIP(hipStreamWaitEvent(ctx->stream, pipe.filled[b], 0));
        launch_decode(buf[b], m, off, fresh.p, first, kept, bad_dev, ctx->stream);
        PLK_HIP(hipGetLastError());
        PLK_HIP(hipEventRecord(pipe.drained[b], ctx->stream));
    }
    unsigned long long bad = KEY_NONE;
    PLK_HIP(hipMemcpyAsync(&bad, bad_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
    PLK_HIP(hipStreamSynchronize(ctx->stream));
    if (bad_out) *bad_out = bad;
    if (bad != KEY_NONE) { set_error("read key err: point not on curve"); return PLK_ERR_FORMAT; }
    PLK_TRY(srs_replace_guard(ctx, "plk_srs_load_key", which));
    key_install_owned(ctx, which, fresh, kept);
    return PLK_OK;                                                            // (`fresh` now holds the previous allocation: freed here)
}

extern "C" int32_t plk_srs_store_key(plk_ctx *ctx, uint32_t flags, const uint8_t g2[256], uint8_t *out, uint64_t cap, uint64_t *len) {
    if (!ctx || !g2 || !len || (flags & ~PLK_KEY_LAGRANGE)) { set_error("plk_srs_store_key: bad argument"); return PLK_ERR_ARG; }
    const ResidentKey &key = ctx->key[(flags & PLK_KEY_LAGRANGE) ? KEY_LAGRANGE : KEY_MONOMIAL];
    const char *pts = (const char *)key.pts;
    const uint64_t n = key.n;
    if (!pts || n == 0) { set_error("plk_srs_store_key: no resident key of that form"); return PLK_ERR_SRS; }
    *len = 8 + 64 * n + 8 + 256;
    if (!out) return PLK_OK;
    if (cap < *len) { set_error("plk_srs_store_key: buffer too small"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    uint64_t chunk; char *buf[2]; unsigned long long *unused;
    PLK_TRY(key_stage(ctx, n, &chunk, &buf[0], &buf[1], &unused));
    KeyPipe pipe;
    PLK_TRY(pipe.open());
    PLK_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 8; i++) out[i] = (uint8_t)(n >> (8 * (7 - i)));
    uint32_t k = 0;
    for (uint64_t off = 0; off < n; off += chunk, k++) {                       // kernel k + 1 beside the download of chunk k
        const uint64_t m = n - off < chunk ? n - off : chunk;
        const int b = k & 1;
        if (k >= 2) PLK_HIP(hipStreamWaitEvent(ctx->stream, pipe.drained[b], 0));
        hipLaunchKernelGGL(g1_encode_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, ctx->stream, (const G1Affine *)(pts + 64 * off), m, (u32x4 *)buf[b]);
        PLK_HIP(hipGetLastError());
        PLK_HIP(hipEventRecord(pipe.filled[b], ctx->stream));
        PLK_HIP(hipStreamWaitEvent(pipe.copy, pipe.filled[b], 0));
        PLK_HIP(hipMemcpyAsync(out + 8 + 64 * off, buf[b], 64 * m, hipMemcpyDeviceToHost, pipe.copy));
        PLK_HIP(hipEventRecord(pipe.drained[b], pipe.copy));
    }
    PLK_HIP(hipStreamSynchronize(pipe.copy));
    PLK_HIP(hipStreamSynchronize(ctx->stream));
    uint8_t *p = out + 8 + 64 * n;
    for (int i = 0; i < 7; i++) p[i] = 0;
    p[7] = 2;
    memcpy(p + 8, g2, 256);
    return PLK_OK;
}

// Crs::<Lagrange>::from_powers (src/plonk.rs:179-185) without leaving the device: the G1 iNTT of the first 2^log_n resident points
// becomes the context's Lagrange-form key (`dump-lagrange` then writes it with plk_srs_store_key)
extern "C" int32_t plk_srs_lagrange_from_powers(plk_ctx *ctx, uint32_t log_n) {
    if (!ctx) { set_error("plk_srs_lagrange_from_powers: bad argument"); return PLK_ERR_ARG; }
    if (log_n > 26) { set_error("g1_intt: size exceeds 2^26"); return PLK_ERR_SIZE; }
    const uint64_t n = 1ull << log_n;
    if (!ctx->srs().pts || ctx->srs().n < n) { set_error("g1_intt: SRS too small"); return PLK_ERR_SRS; }
    if (ctx->lagrange().borrowers.load() > 0) return srs_replace_guard(ctx, "plk_srs_lagrange_from_powers", KEY_LAGRANGE);
    PLK_HIP(hipSetDevice(ctx->device));
    DevBuf fresh;
    struct Drop { DevBuf &b; ~Drop() { b.release(); } } drop{fresh};
    PLK_TRY(fresh.reserve(n * sizeof(G1Affine)));
    PLK_TRY(g1_intt_dev(ctx, reinterpret_cast<const G1Affine *>(ctx->srs().pts), log_n, fresh.as<G1Affine>(), ctx->stream));
    PLK_HIP(hipStreamSynchronize(ctx->stream));
    PLK_TRY(srs_replace_guard(ctx, "plk_srs_lagrange_from_powers", KEY_LAGRANGE));
    key_install_owned(ctx, KEY_LAGRANGE, fresh, n);
    return PLK_OK;
}
