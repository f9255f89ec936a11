// Witness files on the GPU: load_witness_from_array (src/reader.rs:119-175) without a host pass over the elements.
// The file stores an element as 32 little-endian canonical bytes (repr.read_le + Fr::from_repr, src/reader.rs:169-173); the prover
// wants 8 x u32 limbs in Montgomery form.  The bytes ARE the canonical limbs, so decode = range check + one product by R^2 mod r, and
// encode = one product by 1.  One lane owns one element: two dwordx4 loads and two dwordx4 stores with a 32-byte lane stride, every
// byte of every line used.  The 8 x 32-bit layer of field_dev.h does the product (one CIOS multiplication, no conversion of the limb
// width on either side; the 29-bit layer would pay two repackings for the one product).  Against the host-to-device copy of the same
// bytes the kernels are noise (profiles/wtns_ab.txt), so there is no LDS staging and no tuning.
//
// An element is refused exactly when the host parser (parse_wtns_bin, circuit.cpp) refuses it: value >= r.  The verdict of a buffer is
// the LOWEST refused index (atomicMin on one 64-bit word, as g1_decode_kernel), so it does not depend on the launch geometry.
#include "ctx.h"
#include "circuit.h"

namespace plk {

constexpr uint64_t WTNS_NONE = ~0ull;                      // the verdict word while no element has been refused

// true if the limbs are a canonical residue (< r): the subtraction of r borrows out of the top limb
__device__ __forceinline__ bool fr_below_r(const Fr &x) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)x.l[i] - FrParams::P[i] - br; br = (d >> 32) & 1; }
    return br != 0;
}

// bytes: n elements of the file, 16-byte aligned.  Every element is checked; element i is stored to out[i] if i < keep.
__global__ void __launch_bounds__(256) fr_decode_kernel(const u32x4 *__restrict__ bytes, uint64_t n, Fr *__restrict__ out, uint64_t keep,
                                                        unsigned long long *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32x4 lo = bytes[2 * i], hi = bytes[2 * i + 1];
    Fr v;
    v.l[0] = lo.x; v.l[1] = lo.y; v.l[2] = lo.z; v.l[3] = lo.w;
    v.l[4] = hi.x; v.l[5] = hi.y; v.l[6] = hi.z; v.l[7] = hi.w;
    const bool ok = fr_below_r(v);
    if (!ok) atomicMin(bad, (unsigned long long)i);
    if (i < keep) store_fp(&out[i], ok ? from_canonical(v) : Fr::zero());
}

// Montgomery -> 32 little-endian canonical bytes; limbs >= r (never a value this library made) are reduced once first
__global__ void __launch_bounds__(256) fr_encode_kernel(const Fr *__restrict__ in, uint64_t n, u32x4 *__restrict__ bytes) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr v = load_fp(&in[i]);
    reduce_once<FrParams>(v.l);
    v = to_canonical(v);
    bytes[2 * i] = u32x4{v.l[0], v.l[1], v.l[2], v.l[3]};
    bytes[2 * i + 1] = u32x4{v.l[4], v.l[5], v.l[6], v.l[7]};
}

// the lowest index in [first, n) whose element is not a canonical residue -> atomicMin on *bad
__global__ void __launch_bounds__(256) fr_canonical_kernel(const Fr *__restrict__ v, uint64_t first, uint64_t n, unsigned long long *bad) {
    const uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!fr_below_r(load_fp(&v[i]))) atomicMin(bad, (unsigned long long)i);
}

static inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + 255) / 256); }
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

int32_t fr_decode_launch(const void *bytes, uint64_t n, Fr *out, uint64_t keep, unsigned long long *bad, hipStream_t st) {
    if (n == 0) return PLK_OK;
    hipLaunchKernelGGL(fr_decode_kernel, dim3(blocks_of(n)), dim3(256), 0, st, (const u32x4 *)bytes, n, out, keep, bad);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

int32_t fr_canonical_launch(const Fr *v, uint64_t first, uint64_t n, unsigned long long *bad, hipStream_t st) {
    if (n <= first) return PLK_OK;
    hipLaunchKernelGGL(fr_canonical_kernel, dim3(blocks_of(n - first)), dim3(256), 0, st, v, first, n, bad);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

// the payload of a parsed file -> the staging arena (the payload starts at byte 76 of the file: not 16-byte aligned) -> `keep` elements
// of `out`, everything enqueued on st.  The verdict word is the caller's: it has been set to WTNS_NONE on st.
int32_t wtns_payload_to_dev(plk_ctx *ctx, const uint8_t *payload, uint64_t n, Fr *out, uint64_t keep, unsigned long long *bad, hipStream_t st) {
    if (n == 0) return PLK_OK;
    PLK_TRY(ctx->stage.reserve(n * 32));                     // (every earlier user of the arena has waited for its stream before it returned)
    PLK_HIP(hipMemcpyAsync(ctx->stage.p, payload, n * 32, hipMemcpyHostToDevice, st));       // pageable: the caller's buffer is never page-locked
    return fr_decode_launch(ctx->stage.p, n, out, keep, bad, st);
}

}  // namespace plk

using namespace plk;

extern "C" int32_t plk_fr_decode_dev(plk_ctx *ctx, const void *bytes_dev, uint64_t n, void *fr_dev, uint64_t *bad_out, void *stream) {
    if (bad_out) *bad_out = WTNS_NONE;
    if (!ctx || (n && (!bytes_dev || !fr_dev)) || !aligned16(bytes_dev) || !aligned16(fr_dev)) { set_error("plk_fr_decode_dev: bad argument"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    PLK_TRY(ctx->key_bad.reserve(16));
    unsigned long long bad = WTNS_NONE;
    PLK_HIP(hipMemsetAsync(ctx->key_bad.p, 0xff, 8, s));
    PLK_TRY(fr_decode_launch(bytes_dev, n, static_cast<Fr *>(fr_dev), n, ctx->key_bad.as<unsigned long long>(), s));
    PLK_HIP(hipMemcpyAsync(&bad, ctx->key_bad.p, 8, hipMemcpyDeviceToHost, s));
    PLK_HIP(hipStreamSynchronize(s));                        // the verdict is this call's return value
    if (bad_out) *bad_out = bad;
    if (bad != WTNS_NONE) { set_error("read witness failed: not in field"); return PLK_ERR_FORMAT; }
    return PLK_OK;
}

extern "C" int32_t plk_fr_encode_dev(plk_ctx *ctx, const void *fr_dev, uint64_t n, void *bytes_dev, void *stream) {
    if (!ctx || (n && (!bytes_dev || !fr_dev)) || !aligned16(bytes_dev) || !aligned16(fr_dev)) { set_error("plk_fr_encode_dev: bad argument"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    hipLaunchKernelGGL(fr_encode_kernel, dim3(blocks_of(n)), dim3(256), 0, s, (const Fr *)fr_dev, n, (u32x4 *)bytes_dev);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

extern "C" int32_t plk_wtns_decode(plk_ctx *ctx, const uint8_t *data, uint64_t len, void *fr_dev, uint64_t cap, uint64_t *n_out,
                                   uint64_t *bad_out, void *stream) {
    if (bad_out) *bad_out = WTNS_NONE;
    if (n_out) *n_out = 0;
    if (!ctx || !data || !n_out || !aligned16(fr_dev)) { set_error("plk_wtns_decode: bad argument"); return PLK_ERR_ARG; }
    uint64_t n = 0;
    size_t payload = 0;
    if (!wtns_container(data, len, &n, &payload)) return PLK_ERR_FORMAT;      // the container: parse_wtns_bin's checks, order and words
    *n_out = n;
    if (!fr_dev) return PLK_OK;                                              // (nothing of the context has been read so far)
    if (cap < n) { set_error("plk_wtns_decode: the buffer holds " + std::to_string(cap) + " elements, the file " + std::to_string(n)); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    PLK_TRY(ctx->key_bad.reserve(16));
    unsigned long long bad = WTNS_NONE;
    PLK_HIP(hipMemsetAsync(ctx->key_bad.p, 0xff, 8, s));
    PLK_TRY(wtns_payload_to_dev(ctx, data + payload, n, static_cast<Fr *>(fr_dev), n, ctx->key_bad.as<unsigned long long>(), s));
    PLK_HIP(hipMemcpyAsync(&bad, ctx->key_bad.p, 8, hipMemcpyDeviceToHost, s));
    PLK_HIP(hipStreamSynchronize(s));                        // the verdict is this call's return value (and the arena is free again)
    if (bad_out) *bad_out = bad;
    if (bad != WTNS_NONE) { set_error("read witness failed: not in field"); return PLK_ERR_FORMAT; }
    return PLK_OK;
}
