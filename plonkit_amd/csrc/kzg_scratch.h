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

}  // namespace plk
