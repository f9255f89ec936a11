#pragma once
#include "ctx.h"
#include "hostmath.h"
namespace plk {
// Every commitment against a resident key names it: `key` is one of ctx->key (ctx.h), and all the commitment reads of a key.
// enqueue the whole Pippenger pipeline on `stream`; results (window sums) are copied to ctx->pinned
int32_t msm_enqueue(plk_ctx *ctx, ResidentKey &key, const Fr *scalars_dev, uint64_t n, uint64_t base_offset, hipStream_t stream);
// synchronise and fold the window sums on the host
int32_t msm_finish(plk_ctx *ctx, hipStream_t stream, host::HJac *out);
// up to 8 scalar vectors of the same length against the same bases: one pass of every kernel
int32_t msm_enqueue_batch(plk_ctx *ctx, ResidentKey &key, const Fr *const *scalars_dev, uint32_t batch, uint64_t n, uint64_t base_offset, hipStream_t stream);
int32_t msm_finish_batch(plk_ctx *ctx, hipStream_t stream, host::HJac *out);
int32_t ensure_pinned(plk_ctx *ctx, size_t bytes);
// plk_msm_g1_partial_dev, plk_msm_g1_dev and plk_msm_g1_batch_dev (include/plonkit_amd.h) against `key`, ctx and out checked by the caller
int32_t msm_commit_partial(plk_ctx *ctx, ResidentKey &key, const void *scalars_dev, uint64_t n, uint64_t base_offset, plk_g1_jacobian *out, hipStream_t stream);
int32_t msm_commit(plk_ctx *ctx, ResidentKey &key, const void *scalars_dev, uint64_t n, uint64_t base_offset, plk_g1_affine *out, hipStream_t stream);
int32_t msm_commit_many(plk_ctx *ctx, ResidentKey &key, const void *const *scalars_dev, uint32_t count, uint64_t n, uint64_t base_offset, plk_g1_affine *out, hipStream_t stream);

// Commitments against caller-supplied bases (device, the key's in-memory form): out[k] = sum_i scalars_dev[k][i] * bases_dev[i], k < batch.
// Synchronous, ordered after `caller`; refuses (PLK_ERR_ARG) while a commitment is in flight.  batch == 1 takes any length (passes of 2^24
// terms, summed on the host), a batch up to 2^24 terms.  check: *bad = lowest index of a base that is neither (0, 0) nor a curve point with
// coordinates below q, PLK_ERR_FORMAT, and no commitment kernel has run; otherwise *bad = MSM_BASES_NONE.  Reads and writes nothing resident.
constexpr uint64_t MSM_BASES_NONE = ~0ull;
int32_t msm_bases_commit(plk_ctx *ctx, const void *bases_dev, const Fr *const *scalars_dev, uint32_t batch, uint64_t n, bool check, uint64_t *bad,
                         hipStream_t caller, host::HJac *out);
// The converted bases live in ctx->bases_w (grows only).  An entry point that had to grow it beyond 2^20 points' worth gives it back on every
// way out, as the key checks do with the prover's workspace: a one-off sum of 2^24 terms does not leave 1 GiB attached to the context.
struct BasesScratchLoan {
    static constexpr size_t KEEP_BYTES = (size_t)64 << 20;
    plk_ctx *ctx; size_t before;
    explicit BasesScratchLoan(plk_ctx *c) : ctx(c), before(c->bases_w.cap) {}
    // (the commitments that read it have finished: the calls are synchronous; after an error hipFree itself waits for the device)
    ~BasesScratchLoan() { if (ctx->bases_w.cap > before && ctx->bases_w.cap > KEEP_BYTES) ctx->bases_w.release(); }
};
}  // namespace plk
