// Execution context: one GPU, one stream, cached twiddle tables, resident SRS, scratch arenas.
// Stands where bellman_ce's `Worker` stands in the reference (src/plonk.rs:41,47,183).
#pragma once
#include <utility>
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <map>
#include "../../include/plonkit_amd.h"
#include "field_dev.h"
#include "hostmath.h"
#include "msm_plan.h"
#include "ntt_dispatch.h"

namespace plk {

void set_error(const std::string &msg);
int32_t hip_fail(hipError_t e, const char *what, const char *file, int line);

#define PLK_HIP(expr)                                                          \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) return plk::hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)

#define PLK_TRY(expr)                         \
    do {                                      \
        int32_t _rc = (expr);                 \
        if (_rc != PLK_OK) return _rc;        \
    } while (0)

// base^e for e < 2^28 as lo[e & 16383] * hi[e >> 14] (MAX_LOG_N, POW_SPLIT: ntt_dispatch.h)
struct PowTable {
    const Fr *lo = nullptr;
    const Fr *hi = nullptr;
    const uint32_t *hi_sliced = nullptr;     // optional: the hi table as 9 x 29-bit limbs, 48 B per entry (NTT stage twiddles)
    const uint32_t *hi_tw3 = nullptr;        // optional: the hi table as three shifted copies per entry (field29_dev.h mul_tw3), 112 B per entry
};

// grows-only device buffer.  `borrowed`: a view of another context's allocation (plk_ctx_share_srs) — never freed here,
// never grown (reserve() beyond the capacity fails).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool borrowed = false;
    int32_t reserve(size_t bytes);
    void release();
    void borrow(const DevBuf &o) { release(); p = o.p; cap = o.cap; borrowed = o.p != nullptr; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// A resident key: n G1 points on the device, the MSM's fixed-base table of them, and the key's side of a loan (plk_ctx_share_srs).
// A context holds two, plk_ctx::key[KeyForm]: the monomial SRS and the optional Lagrange-form key, Crs<E, CrsForLagrangeForm>
// (L_i(tau)*G), which plk_prove uses for commit_using_values (`prove -l`, src/plonk.rs:138-146).  Whoever commits names the key it
// commits against (msm.h).  A key changes only through the key_* functions below the context.
enum KeyForm : uint32_t { KEY_MONOMIAL = 0, KEY_LAGRANGE = 1, KEY_FORMS = 2 };
struct ResidentKey {
    const void *pts = nullptr;               // device, Montgomery affine, 64 B per point: own.p, the caller's memory (set_dev) or the lender's
    uint64_t n = 0;
    DevBuf own;
    DevBuf w;                                // the same points in the 2^261 Montgomery domain of field29_dev.h (MSM gathers)
    bool w_valid = false;
    uint32_t w_copies = 0;                   // shifted copies 2^(16k) * P held in w (fixed-base table of the MSM)
    bool w_no_inf = false;                   // w holds no point at infinity: established by every build of the table (msm.hip: ensure_base_table), void
                                             // with it (w_valid) — a key can only change through key_install, so it cannot go stale
    bool borrowed = false;                   // borrower: pts and w are the lender's, which a borrower must neither free nor grow
    std::atomic<int> borrowers{0};           // lender: how many contexts hold this key (it may replace the key while none does)
    void void_table() { w_valid = false; w_no_inf = false; if (w.borrowed) w.release(); }
    void release() { own.release(); w.release(); }
};

}  // namespace plk

struct plk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t flag_ready = nullptr;         // the satisfiability verdict of plk_prove has reached `pinned`
    hipEvent_t in_ready = nullptr;           // plk_prove_assembled_dev: the caller's columns are complete on the caller's stream
    int num_cus = 0;
    // NTT tables (device): omega_{2^28} powers forward / inverse, coset generator 7 and 7^-1
    plk::DevBuf tables;
    plk::PowTable tw_fwd, tw_inv;            // omega_{2^28}^{+-e}, external Montgomery form (R = 2^256)
    plk::PowTable tw_fwd_w, tw_inv_w;        // the same powers in the 2^261 domain of field29_dev.h (NTT passes)
    std::map<std::vector<uint32_t>, plk::PowTable> coset_tabs;   // keyed by the 8 limbs of the shift
    std::vector<void *> coset_allocs;
    struct NttDirect { void *buf; size_t bytes; uint64_t used; };   // `used`: value of ntt_direct_clock at the table's last request (eviction order)
    std::map<uint32_t, NttDirect> ntt_direct;                    // ntt.hip: inter-pass twiddle tables by ntt_table_key, capped together (PLK_NTT_DIRECT_CAP_MB)
    uint64_t ntt_direct_clock = 0;
    struct CosetDirect { plk::DevBuf buf; uint32_t log_n = 0; } coset_direct[2];   // ntt.hip: coset-shift powers of the extensions as tables ([1]: inverse)
    std::map<std::vector<uint32_t>, plk::Fr> inv_cache;
    plk::Fr n_inv[plk::MAX_LOG_N + 1];      // 2^-k
    plk::Fr n_inv_w[plk::MAX_LOG_N + 1];    // 2^-k in the 2^261 domain
    plk::DevBuf ntt_scratch[2];              // ping-pong buffers of the NTT passes: [0] main stream, [1] the prover's background stream
    hipStream_t bg_stream = nullptr;         // low-priority stream of the prover: extensions that no challenge waits for
    hipEvent_t bg_go = nullptr, bg_done = nullptr;
    plk::ResidentKey key[plk::KEY_FORMS];    // the SRS and the optional Lagrange-form key
    // MSM: up to three commitments (or batches) may be in flight, each with its own scratch, result buffer and stream:
    // the latency-bound tail of commitment k-1 (bucket reduction) and the digit / partition kernels of k+1 then share the
    // GPU with the accumulation of k, which starts the moment the previous accumulation ends.  A slot is taken lowest
    // index first, so a caller that keeps at most two in flight (the prover) never allocates the third slot's scratch.
    static constexpr uint32_t MSM_SLOTS = plk::MSM_SLOTS;
    struct MsmSlot {
        plk::DevBuf a, b, c, d, e, f;
        void *pinned = nullptr; size_t pinned_cap = 0;
        plk::MsmPlan plan = plk::msm_plan_nothing(0, 1, 0);   // which kernels the commitment it holds was given (msm_plan.h); plan.shape is what plk_msm_last_shape reports
        // what a re-run needs beyond the plan (a short commitment whose bucket lists overflowed: msm_finish_batch)
        const void *bases = nullptr, *scalars[plk::MSM_MAX_BATCH] = {nullptr};
        hipStream_t stream = nullptr;        // the kernels of this commitment; ordered after the caller's stream by `ready`
        hipEvent_t ready = nullptr;
        hipEvent_t acc_done = nullptr;       // recorded behind msm_accumulate: from here on the commitment only runs its latency-bound reduction
        hipEvent_t ev[2] = {nullptr, nullptr};   // optional bracket around msm_accumulate (bench roofline)
        bool busy = false;
        bool acc_no_inf = false;             // msm_accumulate ran without the is_inf(q) test (plk_msm_last_no_inf: diagnostic)
    } slot[MSM_SLOTS];
    uint64_t msm_enq = 0, msm_fin = 0;       // FIFO counters; commitment number k lives in slot[fifo[k % MSM_SLOTS]]
    uint8_t fifo[MSM_SLOTS] = {};
    uint32_t last_slot = 0;                  // slot of the commitment finished last (plk_msm_last_kernel_ms, plk_msm_last_shape)
    uint32_t call_pieces = 0;                // plk_msm_g1_partial_dev: passes of its last call, their length, and msm_fin when it returned
    uint64_t call_piece_terms = 0, call_fin = 0;
    MsmSlot &front_slot() { return slot[fifo[msm_fin % MSM_SLOTS]]; }
    plk::DevBuf bases_w;                     // msm.hip: caller-supplied bases of the current pass in the 2^261 domain (plk_msm_g1_bases*); never kept across calls
    plk::DevBuf prove_ws;                    // workspace of the prover rounds (grows only)
    plk::DevBuf poly_tmp, poly_tmp2;         // scan block totals / evaluation partials
    plk::DevBuf stage;                       // host<->device staging for the host-pointer API
    plk::DevBuf key_bad;                     // keyio.hip: the verdict word of plk_g1_decode_dev (lowest refused index)
    void *pinned = nullptr;                  // small pinned host buffer for results
    size_t pinned_cap = 0;
    void *pinned2 = nullptr;                 // pinned staging of the prover's temporaries
    size_t pinned2_cap = 0;
    plk_transcript_ops tr_ops = {};          // plk_ctx_set_transcript: the caller's Fiat-Shamir transcript for this context's proofs (a copy of the table)
    bool tr_set = false;                     // false: the built-in RollingKeccak
    std::vector<double> timings;
    // intermediate vectors of the last plk_prove, still resident in prove_ws (plk_prove_trace: test / debugging hook)
    struct Trace { const plk::Fr *ptr[12] = {nullptr}; uint64_t len[12] = {0}; bool valid = false; } trace;
    bool ev_on = false;                      // record the per-slot event bracket around msm_accumulate
    float r1cs_ms[4] = {0, 0, 0, 0};         // r1cs_check.hip: kernel times of the last witness check (recorded while ev_on)
    bool r1cs_ms_valid = false;
    float update_ms = 0;                     // srs_update.hip: the kernels of the last plk_srs_update, table fill to last chunk (recorded while ev_on)
    bool update_ms_valid = false;
    float vm_ms[6] = {0, 0, 0, 0, 0, 0};     // verify_many.hip: host flattening (or the front kernel), upload, the three kernels, download of the last plk_verify_many / _packed (recorded while ev_on)
    bool vm_ms_valid = false;
    plk::DevBuf vm_stage;                    // working memory of plk_verify_many_dev / plk_verify_mixed_dev, which do not wait: NOT `stage` (on_ctx_stream, below)
    hipEvent_t vm_in = nullptr, vm_done = nullptr;   // the two events of on_ctx_stream
    plk::DevBuf pair_tab;                    // verify_many.hip: line table of the G2 pair plk_pairing_check_many_dev saw last
    uint8_t pair_g2[256] = {};
    bool pair_tab_valid = false;
    plk::DevBuf kzg_ws;                      // kzg.hip: scratch of the blocking opening calls (grows only; a call that grew it past 64 MiB frees it on return)
    float km_ms[4] = {0, 0, 0, 0};           // kzg_multi.hip: evaluations, h, W, second quotient with W' of the last plk_kzg_open_multi_dev (recorded while ev_on)
    bool km_ms_valid = false;
    plk::DevBuf kzg_vm;                      // kzg.hip: plk_kzg_verify_many_dev's working memory, its own for vm_stage's reason (the call does not wait)
    // kzg_all.hip (all openings on the domain in one pass).  fk_key: DFT_2N of the arranged key, 2N XYZZ points of the 29-bit layer, this
    // context's own even where the key is borrowed or lent; void with the monomial key (key_changed).  fk_ws: scratch of a call (grows only;
    // a call that grew it past 64 MiB frees it on return).
    plk::DevBuf fk_key, fk_ws;
    bool fk_key_valid = false;
    uint32_t fk_key_log_n = 0;
    float fk_ms[5] = {0, 0, 0, 0, 0};        // key transform, Fr NTT, pointwise, inverse, forward + affine of the last plk_kzg_open_all_dev (recorded while ev_on)
    bool fk_ms_valid = false;
    // multi-GPU commitments of the prover (plk_set_commit_shard): global index of the first resident SRS point and
    // the caller's all-ranks combiner for the Jacobian partial sums
    uint64_t shard_first = 0;
    plk_combine_fn combine = nullptr;
    void *combine_user = nullptr;
    uint32_t scatter_open = 0;               // owner-computes mode: vectors of the batch already sent to the workers whose all-gather has not run yet (prover.hip)
    void *comm = nullptr;                    // built-in communicator (plk_comm_init / _tcp, comm.cpp), or null
    std::vector<plk::host::HJac> commit_pieces;   // partial sums of a commitment longer than one MSM call (prover.hip)
    std::vector<plk::host::HJac> commit_done;     // finished commitments of a batch that is processed one at a time
    // plk_ctx_share_srs: a context that proves beside another one on the same GPU borrows that one's resident key(s) and MSM
    // fixed-base table(s) instead of holding a second copy.  The lender counts the borrowers of each key (ResidentKey) and refuses
    // to replace a key while one exists; a borrower drops the loan when it is given a key of its own or destroyed.
    plk_ctx *srs_lender = nullptr;
    bool zombie = false;                     // lender destroyed while borrowers exist: only the lent key and tables are left, freed with the last loan
    plk::ResidentKey &srs() { return key[plk::KEY_MONOMIAL]; }
    plk::ResidentKey &lagrange() { return key[plk::KEY_LAGRANGE]; }
};

namespace plk {
// Every change of a resident key ends in key_install, and with it in key_changed: the key's MSM table is void (a table that was only
// borrowed is let go, not written to when the next one is built), and so is what the context derived from the monomial key.
// Before it, every entry point that replaces a key passes the guard.
int32_t srs_replace_guard(plk_ctx *c, const char *who, KeyForm which = KEY_MONOMIAL);   // runtime.hip: PLK_ERR_ARG while another context borrows that key
// (the monomial key's transform, kzg_all.hip, cannot outlive its key; the buffer stays for the next one)
inline void key_changed(plk_ctx *c, KeyForm which) { if (which == KEY_MONOMIAL) c->fk_key_valid = false; }
// the key is now the n points at `pts`: the key's own buffer filled in place, or memory the caller keeps alive (nullptr, 0: no key)
inline void key_install(plk_ctx *c, KeyForm which, const void *pts, uint64_t n) {
    ResidentKey &k = c->key[which];
    k.pts = pts; k.n = n; k.void_table();
    key_changed(c, which);
}
// the same for a key that was completed beside the old one: `fresh` becomes the key's own buffer and leaves with the old allocation
inline void key_install_owned(plk_ctx *c, KeyForm which, DevBuf &fresh, uint64_t n) {
    std::swap(c->key[which].own, fresh);
    key_install(c, which, c->key[which].own.p, n);
}
inline void key_clear(plk_ctx *c, KeyForm which) { key_install(c, which, nullptr, 0); }
// plk_set_kernel_timing: N events around the stages of a call, created only while ctx->ev_on and destroyed on the way out.  Without
// timing, mark and elapsed do nothing.
template <int N> struct StageTimer {
    hipEvent_t e[N] = {};
    bool on = false;
    StageTimer() = default;
    StageTimer(const StageTimer &) = delete;
    ~StageTimer() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    int32_t start(const plk_ctx *c) {
        if (!c->ev_on) return PLK_OK;
        on = true;
        for (int k = 0; k < N; k++) PLK_HIP(hipEventCreate(&e[k]));
        return PLK_OK;
    }
    int32_t mark(int k, hipStream_t st) { if (on) PLK_HIP(hipEventRecord(e[k], st)); return PLK_OK; }
    int32_t elapsed(int a, int b, float *ms) { if (on) PLK_HIP(hipEventElapsedTime(ms, e[a], e[b])); return PLK_OK; }
};

// The hand-over of a call that returns without waiting (plk_verify_many_dev, plk_verify_mixed_dev, plk_kzg_verify_many_dev): body(st) enqueues
// on the context's stream, after what the caller's stream holds now, and the caller's stream goes on after it; a second such call queues
// behind the first.  Such a call keeps out of the staging arena `stage`, whose users (the blocking calls) each rely on the earlier ones
// having waited, and some of which write it on a stream of the caller's choice.  Its working memory is a buffer of its own, vm_stage or
// kzg_vm, which only kernels on the context's stream touch.  Reserve that buffer BEFORE the hand-over: growing it frees the old block, which
// waits for the device.
template <class Fn> inline int32_t on_ctx_stream(plk_ctx *c, hipStream_t caller, Fn body) {
    const hipStream_t st = c->stream;
    if (caller != st) {
        if (!c->vm_in) PLK_HIP(hipEventCreateWithFlags(&c->vm_in, hipEventDisableTiming));
        if (!c->vm_done) PLK_HIP(hipEventCreateWithFlags(&c->vm_done, hipEventDisableTiming));
        PLK_HIP(hipEventRecord(c->vm_in, caller));
        PLK_HIP(hipStreamWaitEvent(st, c->vm_in, 0));
    }
    PLK_TRY(body(st));
    if (caller != st) {
        PLK_HIP(hipEventRecord(c->vm_done, st));
        PLK_HIP(hipStreamWaitEvent(caller, c->vm_done, 0));
    }
    return PLK_OK;
}
void srs_return_loan(plk_ctx *c);                                 // runtime.hip
void srs_make_loan(plk_ctx *dst, plk_ctx *src);                   // runtime.hip
bool srs_orphan_lender(plk_ctx *c);                               // runtime.hip
}  // namespace plk
