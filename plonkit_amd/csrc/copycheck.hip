// Which copy constraint is broken (plk_sigma_decode_dev, plk_setup_check_permutation, plk_check_copies*, and the failure path of
// plk_prove_assembled*): bellman's prove_by_steps (src/plonk.rs:152-159) takes the caller's sigma and columns on trust, and the only thing
// round 2 can say is that the grand product does not close.  Here sigma is turned back into cells — the inverse of k_sigma_from_index
// (poly.hip), sigma_decode_dev.h — and three exact checks name a place: the lowest cell whose sigma value is no label, the lowest cell that
// is nobody's image, the lowest cell whose value differs from its image's.  Lowest = key row * 4 + col, an atomicMin on a 64-bit word that
// starts as UINT64_MAX (as k_check_gates<true> reports its row).
//
// One lane per cell everywhere.  The decode is ALU-bound (about log_n^2 / 2 Montgomery squarings per value, 32 B read and 4 B written);
// the other three kernels are single passes over 4 B (+ 64 B for the copy check) per cell.
#include "ctx.h"
#include "poly.h"
#include "sigma_decode_dev.h"

namespace plk {

constexpr int PT = 256;
constexpr uint32_t ROW_MASK = 0x3fffffffu;

// base^e from the two-level table (the rule of poly.hip's pow2l_)
struct TablePow {
    PowTable t;
    __device__ __forceinline__ Fr operator()(uint32_t e) const { return mul(load_fp(t.lo + (e & (POW_TAB - 1))), load_fp(t.hi + (e >> POW_SPLIT))); }
};

struct Sigma4 { const Fr *v[4]; };

// idx[col * n + row] <- the cell sigma_col(omega^row) names, or SIGMA_NOT_A_LABEL; *bad (may be null) <- min key of the refused cells
__global__ void __launch_bounds__(PT) k_sigma_decode(Sigma4 sig, uint32_t n, uint32_t log_n, SigmaConsts C, PowTable tw_fwd, PowTable tw_inv, uint32_t *idx,
                                                     unsigned long long *bad) {
    const uint32_t row = blockIdx.x * PT + threadIdx.x, col = blockIdx.y;
    if (row >= n) return;
    const uint32_t p = sigma_decode(load_fp(sig.v[col] + row), log_n, C, TablePow{tw_fwd}, TablePow{tw_inv});
    idx[(size_t)col * n + row] = p;
    if (p == SIGMA_NOT_A_LABEL && bad) atomicMin(bad, (unsigned long long)row * 4 + col);
}

// marks[image of the cell] <- 1.  Lanes that share an image store the same byte; a refused cell has no image.
__global__ void __launch_bounds__(PT) k_mark_images(const uint32_t *idx, uint32_t n, uint8_t *marks) {
    const uint32_t row = blockIdx.x * PT + threadIdx.x, col = blockIdx.y;
    if (row >= n) return;
    const uint32_t p = idx[(size_t)col * n + row];
    if (p == SIGMA_NOT_A_LABEL || (p & ROW_MASK) >= n) return;
    marks[(size_t)(p >> 30) * n + (p & ROW_MASK)] = 1;
}

__global__ void __launch_bounds__(PT) k_unmarked_min(const uint8_t *marks, uint32_t n, unsigned long long *lowest) {
    const uint32_t row = blockIdx.x * PT + threadIdx.x, col = blockIdx.y;
    if (row >= n) return;
    if (!marks[(size_t)col * n + row]) atomicMin(lowest, (unsigned long long)row * 4 + col);
}

// value(cell) against value(image of the cell); the columns are read as zero from `rows` on
__global__ void __launch_bounds__(PT) k_copy_check(const uint32_t *idx, Sigma4 cols, uint32_t n, uint32_t rows, unsigned long long *lowest) {
    const uint32_t row = blockIdx.x * PT + threadIdx.x, col = blockIdx.y;
    if (row >= n) return;
    const uint32_t p = idx[(size_t)col * n + row], col2 = p >> 30, row2 = p & ROW_MASK;
    if (p == SIGMA_NOT_A_LABEL || row2 >= n) return;
    const Fr *src = col2 == 0 ? cols.v[0] : col2 == 1 ? cols.v[1] : col2 == 2 ? cols.v[2] : cols.v[3];
    const Fr mine = row < rows ? load_fp(cols.v[col] + row) : Fr::zero();
    const Fr other = row2 < rows ? load_fp(src + row2) : Fr::zero();
    if (mine != other) atomicMin(lowest, (unsigned long long)row * 4 + col);
}

static int32_t sigma_decode_launch(plk_ctx *ctx, const Fr *const sigma[4], uint32_t log_n, uint32_t *idx, unsigned long long *bad, hipStream_t st) {
    const uint32_t n = 1u << log_n;
    Sigma4 s4;
    for (int j = 0; j < 4; j++) s4.v[j] = sigma[j];
    hipLaunchKernelGGL(k_sigma_decode, dim3((n + PT - 1) / PT, 4), dim3(PT), 0, st, s4, n, log_n, sigma_consts(log_n), ctx->tw_fwd, ctx->tw_inv, idx, bad);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

static int32_t copy_check_enqueue(plk_ctx *ctx, const Fr *const sigma[4], uint32_t log_n, const Fr *const cols[4], uint64_t rows, uint32_t *idx, uint8_t *marks,
                                  unsigned long long *words, hipStream_t st) {
    const uint32_t n = 1u << log_n;
    const dim3 grid((n + PT - 1) / PT, 4), block(PT);
    PLK_HIP(hipMemsetAsync(words, 0xff, 3 * sizeof(unsigned long long), st));
    PLK_HIP(hipMemsetAsync(marks, 0, (size_t)4 * n, st));
    PLK_TRY(sigma_decode_launch(ctx, sigma, log_n, idx, words, st));
    hipLaunchKernelGGL(k_mark_images, grid, block, 0, st, idx, n, marks);
    PLK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_unmarked_min, grid, block, 0, st, marks, n, words + 1);
    PLK_HIP(hipGetLastError());
    if (cols) {
        Sigma4 c4;
        for (int j = 0; j < 4; j++) c4.v[j] = cols[j];
        hipLaunchKernelGGL(k_copy_check, grid, block, 0, st, idx, c4, n, (uint32_t)rows, words + 2);
        PLK_HIP(hipGetLastError());
    }
    return PLK_OK;
}

int32_t copy_check(plk_ctx *ctx, const Fr *const sigma[4], uint32_t log_n, const Fr *const cols[4], uint64_t rows, plk_copy_report *out, hipStream_t st) {
    if (log_n < 1 || log_n > SIGMA_MAX_LOG_N || rows > (1ull << log_n)) { set_error("copy_check: bad argument"); return PLK_ERR_ARG; }
    const uint64_t N = 1ull << log_n;
    // 4N packed cells, 4N mark bytes, the three verdict words (all three kernels run: one round trip whatever the verdict)
    DevBuf buf;
    PLK_TRY(buf.reserve(4 * N * 4 + 4 * N + 64));
    uint32_t *idx = buf.as<uint32_t>();
    uint8_t *marks = reinterpret_cast<uint8_t *>(idx + 4 * N);
    unsigned long long *words = reinterpret_cast<unsigned long long *>(marks + 4 * N);
    unsigned long long got[3] = {~0ull, ~0ull, ~0ull};
    uint32_t image = 0;
    int32_t rc = copy_check_enqueue(ctx, sigma, log_n, cols, rows, idx, marks, words, st);
    if (rc == PLK_OK && hipMemcpyAsync(got, words, sizeof got, hipMemcpyDeviceToHost, st) != hipSuccess) rc = hip_fail(hipGetLastError(), "D2H", __FILE__, __LINE__);
    if (hipStreamSynchronize(st) != hipSuccess && rc == PLK_OK) rc = hip_fail(hipGetLastError(), "sync", __FILE__, __LINE__);
    const bool broken = rc == PLK_OK && got[0] == ~0ull && got[1] == ~0ull && got[2] != ~0ull;
    if (broken) {                                                    // the image of the broken cell
        if (hipMemcpy(&image, idx + (got[2] & 3) * N + (got[2] >> 2), 4, hipMemcpyDeviceToHost) != hipSuccess) rc = hip_fail(hipGetLastError(), "D2H", __FILE__, __LINE__);
    }
    buf.release();
    if (rc != PLK_OK) return rc;
    *out = plk_copy_report{PLK_COPY_OK, 0, 0, 0, 0};
    const int which = got[0] != ~0ull ? 0 : got[1] != ~0ull ? 1 : broken ? 2 : -1;
    if (which < 0) return PLK_OK;
    out->kind = which == 0 ? PLK_COPY_NOT_A_LABEL : which == 1 ? PLK_COPY_NOT_BIJECTIVE : PLK_COPY_BROKEN;
    out->col = (uint32_t)(got[which] & 3); out->row = (uint32_t)(got[which] >> 2);
    if (which == 2) { out->col2 = image >> 30; out->row2 = image & ROW_MASK; }
    return PLK_OK;
}

}  // namespace plk

using namespace plk;

extern "C" int32_t plk_sigma_decode_dev(plk_ctx *ctx, const void *const sigmas_dev[4], uint32_t log_n, void *index_dev, uint64_t *bad_key, void *stream) {
    bool ok = ctx && sigmas_dev && index_dev && log_n >= 1 && log_n <= SIGMA_MAX_LOG_N;
    for (int j = 0; ok && j < 4; j++) ok = sigmas_dev[j] != nullptr;
    if (!ok) { set_error("plk_sigma_decode_dev: bad argument"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const Fr *sig[4];
    for (int j = 0; j < 4; j++) sig[j] = (const Fr *)sigmas_dev[j];
    DevBuf word;
    unsigned long long got = ~0ull;
    if (bad_key) PLK_TRY(word.reserve(64));
    int32_t rc = PLK_OK;
    if (bad_key && hipMemsetAsync(word.p, 0xff, 8, st) != hipSuccess) rc = hip_fail(hipGetLastError(), "memset", __FILE__, __LINE__);
    if (rc == PLK_OK) rc = sigma_decode_launch(ctx, sig, log_n, (uint32_t *)index_dev, word.as<unsigned long long>(), st);
    if (rc == PLK_OK && bad_key && hipMemcpyAsync(&got, word.p, 8, hipMemcpyDeviceToHost, st) != hipSuccess) rc = hip_fail(hipGetLastError(), "D2H", __FILE__, __LINE__);
    if (hipStreamSynchronize(st) != hipSuccess && rc == PLK_OK) rc = hip_fail(hipGetLastError(), "sync", __FILE__, __LINE__);
    word.release();
    if (rc == PLK_OK && bad_key) *bad_key = got;
    return rc;
}
