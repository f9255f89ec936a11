// The scratch of the blocking opening calls (kzg.hip, kzg_multi.hip): ctx->kzg_ws grows only, and a call that grew it past KZ_KEEP gives it
// back on the way out.
#pragma once
#include "ctx.h"
namespace plk {

constexpr size_t KZ_KEEP = (size_t)64 << 20;                    // scratch beyond this is released on return

struct KzgScratch {
    plk_ctx *ctx; hipStream_t st; bool grew = false;
    KzgScratch(plk_ctx *c, hipStream_t s) : ctx(c), st(s) {}
    int32_t reserve(size_t bytes) {
        if (bytes > ctx->kzg_ws.cap) { grew = true; PLK_HIP(hipStreamSynchronize(st)); }
        return ctx->kzg_ws.reserve(bytes);
    }
    ~KzgScratch() { if (grew && ctx->kzg_ws.cap > KZ_KEEP) { (void)hipStreamSynchronize(st); ctx->kzg_ws.release(); } }
};

// what the values routes refuse about the Lagrange-form key (kzg.hip): it is resident and has exactly n = 2^*log_n points, 1 <= *log_n <= 28
int32_t kzg_lagrange_key(plk_ctx *ctx, uint64_t n, uint32_t *log_n);
// what every multi-point call refuses about its polynomials and its context (kzg_multi.hip), with `who` in front
int32_t km_common(const char *who, plk_ctx *ctx, const void *const *polys, uint32_t count, uint32_t max_count, uint64_t n, uint32_t npoints);

}  // namespace plk
