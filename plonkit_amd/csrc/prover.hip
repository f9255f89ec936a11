// Setup polynomials, verification key and the five prover rounds — device resident.
//
// Mirrors (reference file:line):
//   SetupForProver::prepare_setup_for_prover  src/plonk.rs:97-119   -> plk_setup_prepare
//   make_verification_key + vk.write          src/plonk.rs:122-124 ; src/bin/main.rs:501-502 -> plk_setup_write_vk
//   SetupForProver::prove("keccak"), monomial key = prove_by_steps  src/plonk.rs:132-159 -> plk_prove
//   Proof::write                              src/bin/main.rs:407-408 (layout SURVEY.md A.1)
// The protocol (bellman_ce better_cs prover, source absent) is the one recovered in SURVEY.md
// Appendix A.3/A.4 and pinned byte-for-byte by test/circuits/simple/{vk,proof}.bin.
// Everything O(N) runs on the GPU (ntt.hip, msm.hip, poly.hip); the host keeps the transcript,
// a few dozen scalars per round and the circuit synthesis.
// Streams of a proof: ctx->stream carries the round-critical kernels; every commitment runs on its MSM slot's stream
// (msm.hip); ctx->bg_stream (own NTT scratch) carries the work no challenge waits for — the coset-major extensions of the
// wires, z and the public inputs, and the second opening quotient — started by hand behind the accumulation of the commitment
// in flight, so that it fills the latency-bound ends of a commitment instead of standing between two rounds.
#include "ctx.h"
#include "ntt.h"
#include "msm.h"
#include "poly.h"
#include "circuit.h"
#include "keccak.h"
#include "transcript_ops.h"
#include "comm.h"
#include "prover_math.h"
#include <chrono>
#include <memory>
#include <optional>
#include <thread>
#include <mutex>
#include <algorithm>
#include <cstring>

namespace plk {
using namespace host;

static inline Fr to_dev(const HFr &h) { Fr f; memcpy(f.l, h.l, 32); return f; }
int32_t ensure_pinned2(plk_ctx *ctx, size_t bytes);
int32_t fr_canonical_launch(const Fr *v, uint64_t first, uint64_t n, unsigned long long *bad, hipStream_t st);                                   // wtnsio.hip
int32_t wtns_payload_to_dev(plk_ctx *ctx, const uint8_t *payload, uint64_t n, Fr *out, uint64_t keep, unsigned long long *bad, hipStream_t st);   // wtnsio.hip
static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static HFr host_omega(uint32_t log_n) {
    Fr w = ntt_omega(log_n);
    HFr h; memcpy(h.l, w.l, 32); return h;
}
// the combine step of the coset iNTT (poly.h): its constants once, for a setup's cache (round 3) and for plk_icoset4_coset_major_dev
void icoset_constants(uint32_t log_n, HFr c[5]) { icoset_constants_from(host_omega(2), log_n, c); }
int32_t icoset_combine_ext(Fr *data, uint32_t n, const HFr c[5], hipStream_t s) {
    Fr s_w[4];
    for (int k = 0; k < 4; k++) s_w[k] = to_dev(to_w(c[1 + k]));
    return icoset_combine(data, n, to_dev(to_w(c[0])), s_w, s);
}

// KZG commitments of vectors resident on the device: up to 8 over the same SRS prefix share one pass of the MSM
// kernels.  lagrange = commit_using_values: the vectors are evaluations over the domain and the bases the resident
// Lagrange-form key (same group element).
//
// Split form: the commitment's kernels run on their own stream (msm.hip, MsmSlot), so independent work issued on
// ctx->stream between begin and end fills the SIMDs that the bucket-reduction phase leaves idle.
//
// Multi-GPU (plk_set_commit_shard): this rank holds the SRS points [first, first + srs_n) only, commits that index
// range of every vector and hands the Jacobian partial sums to the caller's combiner (all_gather + EC sum over RCCL).
// One MSM call takes at most 2^24 terms (24-bit index field of a bucket entry): longer vectors (domains 2^25, 2^26 —
// SETUP_MAX_POW2 of the reference is 26) are committed in pieces against successive SRS ranges, summed on the host.
static uint64_t msm_piece_terms() {
    static const uint64_t v = [] { const char *e = getenv("PLK_MSM_MAX_TERMS"); uint64_t x = e ? strtoull(e, nullptr, 10) : 0; return x >= MSM_NAIVE_BELOW && x <= MSM_PASS_MAX_TERMS ? x : MSM_PASS_MAX_TERMS; }();
    return v;                                                 // (the environment override exists for the tests)
}
// enqueues the pieces of `cnt` commitments over scalars[lo + ...]; every piece but the last is finished here and summed
// into ctx->commit_pieces, the last one stays in flight (the caller overlaps it and calls commit_end)
static int32_t enqueue_pieces(plk_ctx *ctx, ResidentKey &key, const Fr *const *vecs, uint32_t cnt, uint64_t lo, uint64_t hi, uint64_t first_base) {
    const uint64_t piece = msm_piece_terms();
    ctx->commit_pieces.clear();
    const Fr *shifted[8];
    for (uint64_t off = 0;; off += piece) {
        const uint64_t len = hi - lo - off < piece ? hi - lo - off : piece;
        for (uint32_t k = 0; k < cnt; k++) shifted[k] = vecs[k] + lo + off;
        PLK_TRY(msm_enqueue_batch(ctx, key, shifted, cnt, len, first_base + off, ctx->stream));
        if (off + len >= hi - lo) break;
        HJac j[8];
        PLK_TRY(msm_finish_batch(ctx, nullptr, j));
        if (ctx->commit_pieces.empty()) ctx->commit_pieces.assign(j, j + cnt);
        else for (uint32_t k = 0; k < cnt; k++) ctx->commit_pieces[k] = jac_add(ctx->commit_pieces[k], j[k]);
    }
    return PLK_OK;
}
static int32_t finish_pieces(plk_ctx *ctx, uint32_t cnt, HJac *j) {
    if (ctx->msm_fin != ctx->msm_enq && ctx->front_slot().plan.shape.batch != cnt) {      // never pop somebody else's commitment
        set_error("commitment FIFO out of step: the slot in flight holds a different batch than the prover enqueued"); return PLK_ERR_ARG; }
    PLK_TRY(msm_finish_batch(ctx, nullptr, j));
    if (!ctx->commit_pieces.empty()) {
        for (uint32_t k = 0; k < cnt; k++) j[k] = jac_add(j[k], ctx->commit_pieces[k]);
        ctx->commit_pieces.clear();
    }
    return PLK_OK;
}
static int32_t commit_begin(plk_ctx *ctx, const Fr *const *vecs, uint32_t count, uint64_t n, bool lagrange = false) {
    ResidentKey &key = ctx->key[lagrange ? KEY_LAGRANGE : KEY_MONOMIAL];
    uint64_t lo = 0, hi = n;
    if (ctx->combine) {
        lo = ctx->shard_first < n ? ctx->shard_first : n;
        hi = ctx->shard_first + key.n < n ? ctx->shard_first + key.n : n;
        if (hi < lo) hi = lo;
    }
    const uint64_t first_base = ctx->combine ? 0 : lo;
    ctx->commit_done.clear();
    // owner-computes mode (comm.h): the other ranks do not run this prover — they get their slices of the vectors now, commit them
    // while this rank commits its own, and meet it in commit_end's exchange
    if (comm_scatter_owner(ctx)) {
        if (ctx->shard_first != 0) { set_error("scatter mode: the owner (rank 0) must hold the first slice of the key"); return PLK_ERR_ARG; }
        PLK_TRY(comm_send_work(ctx, reinterpret_cast<const void *const *>(vecs), count, n, key.n, lagrange, ctx->stream));
        ctx->scatter_open = count;                                // the workers now sit in this batch's all-gather: it MUST be run (commit_end, or the FIFO guard)
    }
    // at the largest sizes a batch of commitments would need gigabytes of per-task partial-sum slots (2^26 gates: 16 GiB for
    // four wires, which is what stands between that domain and the 288 GB): one commitment at a time there
    if (count > 1 && hi - lo > msm_piece_terms()) {
        for (uint32_t k = 0; k + 1 < count; k++) {
            HJac j;
            PLK_TRY(enqueue_pieces(ctx, key, vecs + k, 1, lo, hi, first_base));
            PLK_TRY(finish_pieces(ctx, 1, &j));
            ctx->commit_done.push_back(j);
        }
        return enqueue_pieces(ctx, key, vecs + count - 1, 1, lo, hi, first_base);
    }
    return enqueue_pieces(ctx, key, vecs, count, lo, hi, first_base);
}
static int32_t commit_end(plk_ctx *ctx, uint32_t count, HAffine *out) {
    HJac j[8];
    if (!ctx->commit_done.empty()) {                              // the one-at-a-time path of commit_begin
        const uint32_t done = (uint32_t)ctx->commit_done.size();
        for (uint32_t k = 0; k < done; k++) j[k] = ctx->commit_done[k];
        PLK_TRY(finish_pieces(ctx, 1, j + done));
        ctx->commit_done.clear();
    } else PLK_TRY(finish_pieces(ctx, count, j));
    if (ctx->combine) {
        plk_g1_jacobian raw[8];
        for (uint32_t k = 0; k < count; k++) { memcpy(raw[k].x, j[k].x.l, 32); memcpy(raw[k].y, j[k].y.l, 32); memcpy(raw[k].z, j[k].z.l, 32); }
        set_error("");
        ctx->scatter_open = 0;
        const int32_t rc = ctx->combine(ctx->combine_user, raw, count);
        if (rc != PLK_OK) {                                        // (the built-in combiner says why: keep its words)
            const std::string why = plk_last_error();
            set_error(why.empty() ? std::string("commitment combiner (plk_set_commit_shard) failed") : "commitment combiner failed: " + why);
            return rc;
        }
        for (uint32_t k = 0; k < count; k++) { memcpy(j[k].x.l, raw[k].x, 32); memcpy(j[k].y.l, raw[k].y, 32); memcpy(j[k].z.l, raw[k].z, 32); }
    }
    jac_to_affine_batch(j, count, out);                       // one field inversion for the whole batch (13 us each on the host)
    return PLK_OK;
}
static int32_t commit_many(plk_ctx *ctx, const Fr *const *coefs, uint32_t count, uint64_t n, HAffine *out, bool lagrange = false) {
    for (uint32_t done = 0; done < count;) {
        uint32_t b = count - done > 8 ? 8 : count - done;
        PLK_TRY(commit_begin(ctx, coefs + done, b, n, lagrange));
        PLK_TRY(commit_end(ctx, b, out + done));
        done += b;
    }
    return PLK_OK;
}

// plk_comm_serve, the worker side of owner-computes mode: whatever the owner's commit_begin sends is committed against this context's
// slice of the key (commit_begin / commit_end on the received slices: same pieces, same FIFO, same exchange as a replicated rank)
static int32_t serve_impl(plk_ctx *ctx, uint64_t *batches) {
    for (;;) {
        ShardWork w;
        PLK_TRY(comm_recv_work(ctx, &w, ctx->stream));
        if (w.op == SHARD_STOP) return PLK_OK;
        const bool lagrange = w.lagrange != 0;
        if (lagrange && !ctx->lagrange().pts) { set_error("plk_comm_serve: the owner commits against a Lagrange-form key this rank does not hold"); return PLK_ERR_SRS; }
        if (ctx->key[lagrange ? KEY_LAGRANGE : KEY_MONOMIAL].n != w.slice) { set_error("plk_comm_serve: this rank's key slice has a different size than the owner's (every rank holds points [r L, (r+1) L))"); return PLK_ERR_SRS; }
        const Fr *vecs[8];
        static const Fr none{};
        for (uint32_t k = 0; k < w.count; k++) vecs[k] = w.len ? static_cast<const Fr *>(w.vec[k]) : &none;
        // (the received slices ARE this rank's index range: commit them as vectors of their own length from index 0)
        const uint64_t keep_first = ctx->shard_first;
        ctx->shard_first = 0;
        int32_t rc = commit_begin(ctx, vecs, w.count, w.len, lagrange);
        HAffine out[8];
        if (rc == PLK_OK) rc = commit_end(ctx, w.count, out);
        ctx->shard_first = keep_first;
        PLK_TRY(rc);
        if (batches) ++*batches;
    }
}

// plk_prove / plk_setup_write_vk own the two-slot commitment FIFO for the duration of the call: it must be empty on
// entry (a commitment the caller enqueued with plk_msm_g1_enqueue_dev and never finished would otherwise be popped as
// one of the prover's), and whatever an early error return leaves in flight is drained before the call returns.
static int32_t fifo_must_be_empty(plk_ctx *ctx, const char *who) {
    if (ctx->msm_enq == ctx->msm_fin) return PLK_OK;
    set_error(std::string(who) + ": a commitment enqueued with plk_msm_g1_enqueue_dev is still in flight (call plk_msm_g1_finish first)");
    return PLK_ERR_ARG;
}
struct FifoGuard {
    plk_ctx *ctx;
    explicit FifoGuard(plk_ctx *c) : ctx(c) {}
    ~FifoGuard() {
        if (ctx->msm_fin != ctx->msm_enq) {
            const std::string keep = plk_last_error();               // the drain must not replace the error being returned
            while (ctx->msm_fin != ctx->msm_enq) { HJac j[8]; (void)msm_finish_batch(ctx, nullptr, j); }
            set_error(keep);
        }
        ctx->commit_done.clear(); ctx->commit_pieces.clear();
        // Owner-computes mode: a batch went out to the workers (commit_begin) and the call is returning without commit_end — "must satisfy",
        // a failed PLK_TRY in between.  The workers are committing their slices and will enter the batch's all-gather; if the owner never does,
        // they sit there for the exchange deadline (180 s) and the owner's next broadcast meets their all-gather as a mismatched collective.
        // Run the exchange with empty sums (nobody reads the result): owner and workers stay in step, the communicator stays usable.
        if (ctx->scatter_open && ctx->combine) {
            const std::string keep = plk_last_error();
            plk_g1_jacobian raw[8];
            memset(raw, 0, sizeof raw);
            (void)ctx->combine(ctx->combine_user, raw, ctx->scatter_open);
            set_error(keep);
        }
        ctx->scatter_open = 0;
    }
};

struct Arena {
    DevBuf *buf; size_t off = 0;
    template <class T> T *take(size_t count) {
        size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        T *p = reinterpret_cast<T *>((char *)buf->p + off);
        off += bytes;
        return p;
    }
};

}  // namespace plk

struct plk_setup {
    uint64_t n = 0, N = 0, num_inputs = 0, n_real = 0, num_vars = 0, num_gates = 0;
    uint32_t log_n = 0;
    plk::DevBuf store;                     // one allocation holding everything below
    plk::Fr *sel_coef[7] = {nullptr}, *sel_vals[7] = {nullptr}, *sig_coef[4] = {nullptr}, *sig_vals[4] = {nullptr};
    uint32_t *gate_vars[4] = {nullptr};
    // coset LDEs (4N evaluations on 7*<omega_4N>) of the 7 selectors, 4 sigmas and L_0: circuit constants,
    // computed by the first proof and kept (the reference recomputes them in every prove_by_steps call
    // because plonkit passes `None` precomputations, src/plonk.rs:156; the values are identical)
    mutable plk::DevBuf lde_store;
    mutable plk::Fr *lde[13] = {nullptr};       // 7 selectors, 4 sigma, L0 (pre-scaled, see QuotientArgs), coset points
    mutable bool lde_ready = false;
    mutable bool zh_inv_ready = false;
    mutable plk::HFr zh_inv[4];
    mutable plk::HFr icoset_c[5];            // i^-1 (i = omega_4) and 7^(-N c) / 4, c = 0..3: constants of the coset iNTT's combine step
    mutable std::mutex lazy_mu;              // the cached extensions and constants above are filled by the FIRST proof: one setup may be
                                             // proved from several contexts / host threads at once (SetupForProver::prove takes &self)
    uint64_t num_circuit_vars = 0;         // circom wires; temporaries follow
    std::vector<plk::WitnessOp> ops;       // linear forms defining the transpiler's temporaries
    bool ops_independent = false;          // no temporary reads another temporary -> order-free evaluation
    bool ops_chained = false;              // a temporary reads at most its immediate predecessor (partial-sum chains of long linear
                                           // combinations): evaluated on the device run by run (run_start = first temporary of every run)
    std::vector<uint32_t> run_start;
    plk::DevBuf ops_dev, terms_dev, runs_dev;   // the records on the device (when ops_independent or ops_chained): evaluated there
    std::vector<plk::WitnessTerm> op_terms;
    plk::big_vector<plk::HFr> h_cols;      // host phase only: 7 selector columns x N, until plk_setup_upload
    plk::big_vector<uint32_t> h_vars;      // host phase only: 4 variable-index columns x N
    bool from_polys = false;               // plk_setup_from_polynomials: selectors and sigmas given, no gate structure (gate_vars, ops)
};

using namespace plk;

void plk_circuit_unregister(plk_circuit *c) {
    if (c->witness_registered) { (void)hipHostUnregister((void *)c->witness.data()); c->witness_registered = false; }
}

extern "C" {

uint64_t plk_setup_domain_size(const plk_setup *s) { return s ? s->N : 0; }
void plk_setup_free(plk_setup *s) { if (s) { s->store.release(); s->lde_store.release(); s->ops_dev.release(); s->terms_dev.release(); s->runs_dev.release(); delete s; } }

// the domain size N (and log2 N) a circuit's setup will have — transpile only (pure CPU, ~18 ms at 2^20 gates), no columns, no device work: what
// `dump-lagrange` needs of prepare_setup_for_prover (src/bin/main.rs:360-381 builds the whole setup to read setup.n from it)
int32_t plk_circuit_domain_size(const plk_circuit *c, uint64_t *n_out) {
    if (!c || !n_out) { set_error("plk_circuit_domain_size: bad argument"); return PLK_ERR_ARG; }
    return guarded("plk_circuit_domain_size", PLK_ERR_ARG, [&]() -> int32_t {
        Transpiled T;
        T.collect_stats = false;
        if (!transpile(c->r1cs, nullptr, &T)) return PLK_ERR_UNSAT;
        const uint64_t n_real = (uint64_t)(c->r1cs.num_inputs - 1) + T.num_gates;
        uint64_t N = 1; uint32_t log_n = 0;
        while (N < n_real + 1) { N <<= 1; log_n++; }
        if (log_n + 2 > MAX_LOG_N) { set_error("setup power of two is not in the correct range"); return PLK_ERR_SIZE; }
        *n_out = N;
        return PLK_OK;
    });
}

// SetupForProver::prepare_setup_for_prover in two phases, so that a host program can run the first one (pure CPU:
// transpile, selector / variable-index columns) while the GPU side of its start-up is still under way on another thread
// (HIP initialisation, key upload, MSM table — the `plonkit` binary does exactly that), and the second one when both are done.
static int32_t setup_host_impl(const plk_circuit *c, plk_setup **out) {
    if (!c || !out) { set_error("plk_setup_prepare: bad argument"); return PLK_ERR_ARG; }
    *out = nullptr;
    const bool timing = getenv("PLK_CLI_TIMING") != nullptr;     // phase times of the setup on stderr (tools/cli_scale.sh)
    double t_last = now_ms();
    auto mark = [&](const char *what) { if (timing) { double t = now_ms(); fprintf(stderr, "[timing]   setup: %-22s +%.3f s\n", what, (t - t_last) / 1e3); t_last = t; } };
    Transpiled T;
    T.collect_stats = false;                                     // a million std::string names are only wanted by `analyse`
    if (!transpile(c->r1cs, nullptr, &T)) return PLK_ERR_UNSAT;
    mark("transpile");
    std::unique_ptr<plk_setup> S(new plk_setup());
    S->num_inputs = c->r1cs.num_inputs - 1;
    S->num_gates = T.num_gates;
    S->n_real = S->num_inputs + T.num_gates;
    S->num_vars = T.num_vars;
    uint64_t N = 1; uint32_t log_n = 0;
    while (N < S->n_real + 1) { N <<= 1; log_n++; }
    if (log_n + 2 > MAX_LOG_N) { set_error("setup power of two is not in the correct range"); return PLK_ERR_SIZE; }   // src/plonk.rs:109-112
    S->N = N; S->n = N - 1; S->log_n = log_n;
    S->num_circuit_vars = c->r1cs.num_variables;
    S->ops.swap(T.ops); S->op_terms.swap(T.op_terms);
    S->ops_independent = true;
    for (const WitnessTerm &t : S->op_terms) if (t.var >= c->r1cs.num_variables) { S->ops_independent = false; break; }
    if (!S->ops_independent) {
        // long linear combinations: temporary i (a partial sum) reads temporary i - 1 and circom wires only -> runs
        const uint64_t ncv0 = c->r1cs.num_variables;
        S->ops_chained = true;
        for (size_t i = 0; i < S->ops.size() && S->ops_chained; i++) {
            bool continues = false;
            for (uint32_t k = 0; k < S->ops[i].count; k++) {
                const uint32_t v = S->op_terms[S->ops[i].first + k].var;
                if (v < ncv0) continue;
                if (i > 0 && v == ncv0 + i - 1) continues = true;
                else { S->ops_chained = false; break; }
            }
            if (!continues) S->run_start.push_back((uint32_t)i);
        }
        if (!S->ops_chained) std::vector<uint32_t>().swap(S->run_start);
    }
    // rows of the trace: one gate per public input first (q_a = -1), then the transpiler's gates, then padding with the dummy
    // variable.  The gate pieces are read once, piece-parallel, straight into the seven selector columns and the four
    // variable-index columns.
    const size_t n_in = S->num_inputs, n_rows = n_in + T.num_gates;
    S->h_cols.resize((size_t)7 * N);
    S->h_vars.resize((size_t)4 * N);
    HFr *cols = S->h_cols.data(); uint32_t *vars = S->h_vars.data();
    const HFr minus_one = -HFr::one();
    for (size_t r = 0; r < n_in; r++) {
        for (int k = 0; k < 7; k++) cols[(size_t)k * N + r] = k == 0 ? minus_one : HFr::zero();
        vars[r] = (uint32_t)(r + 1); vars[N + r] = vars[2 * N + r] = vars[3 * N + r] = 0;
    }
    parallel_for(T.pieces.size(), 1, [&](size_t lo, size_t hi) {
        for (size_t p = lo; p < hi; p++) {
            const big_vector<Gate> &gs = T.pieces[p];
            const uint32_t shift = T.tmp_shift[p], first_tmp = (uint32_t)T.first_tmp;
            size_t r = n_in + T.gate0[p];
            for (size_t i = 0; i < gs.size(); i++, r++) {
                const Gate &g = gs[i];
                for (int k = 0; k < 7; k++) cols[(size_t)k * N + r] = g.q[k];
                for (int j = 0; j < 4; j++) vars[(size_t)j * N + r] = g.v[j] >= first_tmp ? g.v[j] + shift : g.v[j];
            }
        }
    });
    parallel_for(N - n_rows, 1 << 15, [&](size_t lo, size_t hi) {
        for (size_t r = n_rows + lo; r < n_rows + hi; r++) {
            for (int k = 0; k < 7; k++) cols[(size_t)k * N + r] = HFr::zero();
            for (int j = 0; j < 4; j++) vars[(size_t)j * N + r] = 0;
        }
    });
    mark("columns (host fill)");
    *out = S.release();
    return PLK_OK;
}

// The copy-constraint permutation of a setup from its 4 x N variable-index table: idx[col * N + row] = col' << 30 | row', the successor of
// every occurrence (perm.hip), and, where sig_vals is given, sigma_col(omega^row) = k_col' * omega^row' (k = 1, 5, 7, 10).  The one place
// that does this: the setup and plk_setup_permutation_dev both call it.  idx is the caller's (4N words); the sigma kernels are enqueued on
// st and read idx, so the caller synchronises before releasing it.
static int32_t setup_permutation(plk_ctx *ctx, const uint32_t *const vars[4], uint32_t log_n, uint64_t num_vars, uint32_t *idx, Fr *const sig_vals[4], hipStream_t st) {
    const uint64_t N = 1ull << log_n;
    PLK_TRY(build_permutation_index(ctx, vars, (uint32_t)N, num_vars, idx, st));
    if (!sig_vals) return PLK_OK;
    Fr kk[4];
    for (int j = 0; j < 4; j++) kk[j] = from_u64<FrParams>(NON_RESIDUES[j]);
    for (int j = 0; j < 4; j++) PLK_TRY(sigma_from_index(sig_vals[j], idx + (size_t)j * N, (uint32_t)N, log_n, ctx->tw_fwd, kk, st));
    return PLK_OK;
}

static int32_t setup_upload_impl(plk_ctx *ctx, plk_setup *S) {
    if (!ctx || !S) { set_error("plk_setup_upload: bad argument"); return PLK_ERR_ARG; }
    if (S->store.p) return PLK_OK;                               // already resident
    if (S->h_cols.empty()) { set_error("plk_setup_upload: the host phase has not run"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    const bool timing = getenv("PLK_CLI_TIMING") != nullptr;
    double t_last = now_ms();
    auto mark = [&](const char *what) { if (timing) { double t = now_ms(); fprintf(stderr, "[timing]   setup: %-22s +%.3f s\n", what, (t - t_last) / 1e3); t_last = t; } };
    const uint64_t N = S->N; const uint32_t log_n = S->log_n;
    static_assert(sizeof(WitnessOp) == 40 && sizeof(WitnessTerm) == 40, "records are uploaded as they are (poly.hip)");
    hipStream_t st = ctx->stream;
    auto fail = [&](int32_t code) { S->store.release(); S->ops_dev.release(); S->terms_dev.release(); S->runs_dev.release(); return code; };
    int32_t rc;
    if (S->ops_chained && !S->ops.empty()) {
        if ((rc = S->runs_dev.reserve(S->run_start.size() * sizeof(uint32_t))) != PLK_OK) return fail(rc);
        if (hipMemcpyAsync(S->runs_dev.p, S->run_start.data(), S->run_start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(hip_fail(hipGetLastError(), "H2D witness runs", __FILE__, __LINE__));
    }
    if ((S->ops_independent || S->ops_chained) && !S->ops.empty()) {                     // temporaries will be evaluated on the device
        if ((rc = S->ops_dev.reserve(S->ops.size() * sizeof(WitnessOp))) != PLK_OK) return fail(rc);
        if ((rc = S->terms_dev.reserve(S->op_terms.size() * sizeof(WitnessTerm) + 8)) != PLK_OK) return fail(rc);
        if (hipMemcpyAsync(S->ops_dev.p, S->ops.data(), S->ops.size() * sizeof(WitnessOp), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(S->terms_dev.p, S->op_terms.data(), S->op_terms.size() * sizeof(WitnessTerm), hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(hip_fail(hipGetLastError(), "H2D witness ops", __FILE__, __LINE__));
    }
    Arena A{&S->store};
    size_t total = 22 * ((N * sizeof(Fr) + 255) & ~(size_t)255) + 4 * ((N * 4 + 255) & ~(size_t)255);
    if ((rc = S->store.reserve(total)) != PLK_OK) return fail(rc);
    for (int k = 0; k < 7; k++) S->sel_coef[k] = A.take<Fr>(N);
    for (int k = 0; k < 7; k++) S->sel_vals[k] = A.take<Fr>(N);
    for (int j = 0; j < 4; j++) S->sig_coef[j] = A.take<Fr>(N);
    for (int j = 0; j < 4; j++) S->sig_vals[j] = A.take<Fr>(N);
    for (int j = 0; j < 4; j++) S->gate_vars[j] = A.take<uint32_t>(N);
    // the columns are uploaded back to back and interpolated as they land
    for (int j = 0; j < 4; j++)
        if (hipMemcpyAsync(S->gate_vars[j], S->h_vars.data() + (size_t)j * N, N * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail(hip_fail(hipGetLastError(), "H2D vars", __FILE__, __LINE__));
    for (int k = 0; k < 7; k++) {
        if (hipMemcpyAsync(S->sel_vals[k], S->h_cols.data() + (size_t)k * N, N * sizeof(Fr), hipMemcpyHostToDevice, st) != hipSuccess) return fail(hip_fail(hipGetLastError(), "H2D selector", __FILE__, __LINE__));
        if (hipMemcpyAsync(S->sel_coef[k], S->sel_vals[k], N * sizeof(Fr), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(hip_fail(hipGetLastError(), "D2D selector", __FILE__, __LINE__));
        if ((rc = ntt_dev(ctx, S->sel_coef[k], log_n, true, nullptr, st)) != PLK_OK) return fail(rc);
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail(hip_fail(hipGetLastError(), "sync", __FILE__, __LINE__));
    big_vector<HFr>().swap(S->h_cols);                           // the host columns go away here
    big_vector<uint32_t>().swap(S->h_vars);
    mark("selectors (upload + 7 iNTT)");
    // the permutation (rotate-left over each variable's occurrences) from the variable-index table, on the device (perm.hip)
    {
        DevBuf idx_buf;
        if ((rc = idx_buf.reserve((size_t)4 * N * 4)) != PLK_OK) return fail(rc);
        if ((rc = setup_permutation(ctx, S->gate_vars, log_n, S->num_vars, idx_buf.as<uint32_t>(), S->sig_vals, st)) != PLK_OK) { idx_buf.release(); return fail(rc); }
        // one launch per pass for the four of them where the batch scratch is small; above, each column is transformed behind its own copy
        const bool singly = ntt_batch_per_launch(NTT_BATCH_PROVER, log_n) == 1;
        for (int j = 0; j < 4; j++) {
            if (hipMemcpyAsync(S->sig_coef[j], S->sig_vals[j], N * sizeof(Fr), hipMemcpyDeviceToDevice, st) != hipSuccess) { idx_buf.release(); return fail(hip_fail(hipGetLastError(), "D2D sigma", __FILE__, __LINE__)); }
            if (singly && (rc = ntt_columns_dev(ctx, &S->sig_coef[j], 1, log_n, true, st)) != PLK_OK) { idx_buf.release(); return fail(rc); }
        }
        if (!singly && (rc = ntt_columns_dev(ctx, S->sig_coef, 4, log_n, true, st)) != PLK_OK) { idx_buf.release(); return fail(rc); }
        hipError_t e = hipStreamSynchronize(st);
        idx_buf.release();
        if (e != hipSuccess) return fail(hip_fail(e, "sync", __FILE__, __LINE__));
    }
    mark("permutation (device sort + 4 iNTT)");
    return PLK_OK;
}

static int32_t setup_prepare_impl(plk_ctx *ctx, const plk_circuit *c, plk_setup **out) {
    if (!ctx || !c || !out) { set_error("plk_setup_prepare: bad argument"); return PLK_ERR_ARG; }
    plk_setup *S = nullptr;
    PLK_TRY(setup_host_impl(c, &S));
    const int32_t rc = setup_upload_impl(ctx, S);
    if (rc != PLK_OK) { plk_setup_free(S); *out = nullptr; return rc; }
    *out = S;
    return PLK_OK;
}

static void put_u64(std::vector<uint8_t> &b, uint64_t v) { for (int i = 7; i >= 0; i--) b.push_back((uint8_t)(v >> (8 * i))); }
static void put_g1(std::vector<uint8_t> &b, const HAffine &p) { uint8_t t[64]; g1_to_bytes(p, t); b.insert(b.end(), t, t + 64); }
static void put_fr(std::vector<uint8_t> &b, const HFr &v) { uint8_t t[32]; v.to_be_bytes(t); b.insert(b.end(), t, t + 32); }

static int32_t setup_write_vk_impl(plk_ctx *ctx, const plk_setup *s, const uint8_t g2_bytes[256], uint8_t *out, uint64_t cap, uint64_t *len) {
    if (!ctx || !s || !g2_bytes || !out || !len) { set_error("plk_setup_write_vk: bad argument"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    if (!s->store.p) { set_error("plk_setup_write_vk: the setup is not on the device yet (plk_setup_upload)"); return PLK_ERR_ARG; }
    PLK_TRY(fifo_must_be_empty(ctx, "plk_setup_write_vk"));
    FifoGuard fifo_guard(ctx);
    std::vector<uint8_t> b;
    put_u64(b, s->n); put_u64(b, s->num_inputs);
    HAffine cm[11];
    {
        const Fr *polys[11];
        for (int k = 0; k < 7; k++) polys[k] = s->sel_coef[k];
        for (int j = 0; j < 4; j++) polys[7 + j] = s->sig_coef[j];
        PLK_TRY(commit_many(ctx, polys, 11, s->N, cm));
    }
    put_u64(b, 6);
    for (int k = 0; k < 6; k++) put_g1(b, cm[k]);
    put_u64(b, 1);
    put_g1(b, cm[6]);
    put_u64(b, 4);
    for (int j = 0; j < 4; j++) put_g1(b, cm[7 + j]);
    put_u64(b, 3);
    for (int j = 1; j < 4; j++) put_fr(b, HFr::from_u64(NON_RESIDUES[j]));
    b.insert(b.end(), g2_bytes, g2_bytes + 256);
    *len = b.size();
    if (b.size() > cap) { set_error("plk_setup_write_vk: buffer too small"); return PLK_ERR_ARG; }
    memcpy(out, b.data(), b.size());
    return PLK_OK;
}

int32_t plk_prove_timings(const plk_ctx *ctx, double *out_ms, uint32_t cap, uint32_t *count) {
    if (!ctx || !count) { set_error("plk_prove_timings: bad argument"); return PLK_ERR_ARG; }
    *count = (uint32_t)ctx->timings.size();
    for (uint32_t i = 0; i < *count && i < cap && out_ms; i++) out_ms[i] = ctx->timings[i];
    return PLK_OK;
}

// ---- the prover's workspace and its two front ends
// Everything of a proof lives in ctx->prove_ws; d_values (the witness by variable index) only on the circuit path.
struct ProveWs {
    Fr *d_values = nullptr, *w_vals[4] = {}, *w_coef[4] = {};
    Fr *z_coef = nullptr, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *r_poly = nullptr, *agg = nullptr, *pi_coef = nullptr, *l0_coef = nullptr;
    Fr *ext[18] = {}, *t_ext = nullptr, *tab[4] = {}, *d_results = nullptr;
    uint32_t *d_flag = nullptr;
    bool direct_pi = false;
};
static int32_t prove_workspace(plk_ctx *ctx, const plk_setup *S, uint64_t num_vars, ProveWs *W) {
    const uint64_t N = S->N, M = 4 * N;
    const size_t NB = (N * sizeof(Fr) + 255) & ~(size_t)255, MB = (M * sizeof(Fr) + 255) & ~(size_t)255;
    const size_t TB = ((size_t)2 * POW_TAB * sizeof(Fr) + 255) & ~(size_t)255;
    const size_t VB = (num_vars * sizeof(Fr) + 255) & ~(size_t)255;
    const bool direct_pi = S->num_inputs <= QUOTIENT_MAX_DIRECT_PI;       // few inputs: PI comes from the cached L0 vector inside the quotient kernel
    W->direct_pi = direct_pi;
    PLK_TRY(ctx->prove_ws.reserve(VB + 16 * NB + (direct_pi ? 6 : 7) * MB + 4 * TB + 8192));   // 5 extensions (+ PI) + the quotient
    Arena A{&ctx->prove_ws};
    W->d_values = A.take<Fr>(num_vars);
    for (int j = 0; j < 4; j++) { W->w_vals[j] = A.take<Fr>(N); W->w_coef[j] = A.take<Fr>(N); }
    W->z_coef = A.take<Fr>(N); W->t1 = A.take<Fr>(N); W->t2 = A.take<Fr>(N); W->t3 = A.take<Fr>(N);
    W->r_poly = A.take<Fr>(N); W->agg = A.take<Fr>(N); W->pi_coef = A.take<Fr>(N); W->l0_coef = A.take<Fr>(N);
    for (int k = 0; k < 18; k++) W->ext[k] = nullptr;
    for (int k = 0; k < 5; k++) W->ext[k] = A.take<Fr>(M);       // w0..w3, z
    if (!direct_pi) W->ext[16] = A.take<Fr>(M);                    // PI
    W->t_ext = A.take<Fr>(M);
    for (int k = 0; k < 4; k++) W->tab[k] = A.take<Fr>(2 * POW_TAB);
    W->d_results = A.take<Fr>(16);
    W->d_flag = A.take<uint32_t>(64);
    return PLK_OK;
}

// What a front end hands to the rounds: w_vals / w_coef of the workspace hold the wire values (w_coef still to be interpolated in place),
// the satisfiability verdict is on its way to ctx->pinned behind ctx->flag_ready, and the public inputs are known — or, for columns
// that live on the device, on their way to inputs_pinned behind the same event.
struct ProveFront {
    std::vector<HFr> inputs;
    const HFr *inputs_pinned = nullptr;
    bool assembled = false;                  // verdict layout: circuit = one flag word; assembled = ingest_columns' two words
    bool close_perm = false;                 // sigma came from the caller: check that the permutation argument closes (round 2)
    int wire_check = 0;                      // circuit verdict layout, second word: 1 = lowest wire that is not canonical, 2 = lowest file element >= r
    uint64_t wire_bad = ~0ull;               // what that word held
    const char *who = "plk_prove";
    double t_prev = 0;                       // plk_prove_timings: start of the phase in progress
};

// the verdict of the front end's checks, read after round 1 has been enqueued (before any commitment is used)
static int32_t front_verdict(plk_ctx *ctx, const plk_setup *S, ProveFront &F) {
    const volatile uint32_t *flag = reinterpret_cast<volatile uint32_t *>(ctx->pinned);
    if (F.assembled) {
        if (const uint32_t bad = flag[0]) {
            std::string which;
            for (int j = 0; j < 4; j++) if (bad >> j & 1) { which += which.empty() ? "" : ", "; which += "abcd"[j]; }
            set_error("plk_prove_assembled: column " + which + " holds an element that is not a canonical residue (limbs >= r)");
            return PLK_ERR_ARG;
        }
        if (const uint32_t f = flag[1]) {
            set_error("must satisfy: the assembled columns fail the gate equation at row " + std::to_string(S->N - f) + " (the lowest failing row)");
            return PLK_ERR_UNSAT;
        }
    } else {
        if (F.wire_check) {
            F.wire_bad = *reinterpret_cast<const volatile uint64_t *>(flag + 2);
            if (F.wire_bad != ~0ull && F.wire_check == 2) { set_error("read witness failed: not in field"); return PLK_ERR_FORMAT; }
            if (F.wire_bad != ~0ull) {
                set_error(std::string(F.who) + ": wire " + std::to_string(F.wire_bad) + " holds an element that is not a canonical residue (limbs >= r)");
                return PLK_ERR_ARG;
            }
        }
        if (flag[0]) { set_error("must satisfy: witness does not satisfy the circuit"); return PLK_ERR_UNSAT; }
    }
    if (F.inputs_pinned) F.inputs.assign(F.inputs_pinned, F.inputs_pinned + S->num_inputs);
    return PLK_OK;
}

// round 2's "copy constraints" message ends with what copy_check (copycheck.hip) found on the columns of the failed proof
static void append_copy_report(std::string &msg, const plk_copy_report &r) {
    auto cell = [](uint32_t col, uint32_t row) { return std::string(1, "abcd"[col & 3]) + "[" + std::to_string(row) + "]"; };
    if (r.kind == PLK_COPY_BROKEN) msg += "; first broken copy: cell " + cell(r.col, r.row) + " and its image " + cell(r.col2, r.row2) + " hold different values";
    else if (r.kind == PLK_COPY_NOT_BIJECTIVE) msg += "; sigma is not a permutation: cell " + cell(r.col, r.row) + " is the image of no cell";
    else if (r.kind == PLK_COPY_NOT_A_LABEL) msg += "; sigma is not a permutation: its value at cell " + cell(r.col, r.row) + " is not a cell label";
}

// ---- the background lane of a proof
// The extensions that no challenge waits for (wires, z, public inputs: round-3 inputs) run on a low-priority stream of
// their own with their own NTT scratch: they fill the SIMDs that the latency-bound ends of a commitment leave idle
// without standing between two rounds — on the main stream round 2 queued up behind the four wire extensions, which
// in turn were starved by the accumulation they shared the GPU with (round 1: 6.4-7.0 ms).  Up to the 2^24 domain (a
// second 4N scratch above that is memory better spent elsewhere); PLK_PROVE_BG=0 restores the single stream: then the
// lane IS the main stream and every operation below is a no-op.
struct BgLane {
    plk_ctx *ctx = nullptr;
    bool on = false;
    bool armed = false;                      // work of the lane may still be writing into the arena: an early return waits for it
    ~BgLane() { if (armed && on && ctx->bg_stream) (void)hipStreamSynchronize(ctx->bg_stream); }
    hipStream_t stream() const { return on ? ctx->bg_stream : ctx->stream; }
    uint32_t ntt_lane() const { return on ? 1 : 0; }          // which NTT scratch its transforms use
    int32_t open(plk_ctx *c, uint32_t log_n) {
        static const bool bg_env = [] { const char *e = getenv("PLK_PROVE_BG"); return !(e && e[0] == '0'); }();
        ctx = c;
        on = armed = bg_env && log_n <= 24;
        if (on && !ctx->bg_stream) {
            int lo_prio = 0, hi_prio = 0;
            PLK_HIP(hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio));
            PLK_HIP(hipStreamCreateWithPriority(&ctx->bg_stream, hipStreamNonBlocking, lo_prio));
            PLK_HIP(hipEventCreateWithFlags(&ctx->bg_go, hipEventDisableTiming));
            PLK_HIP(hipEventCreateWithFlags(&ctx->bg_done, hipEventDisableTiming));
        }
        return PLK_OK;
    }
    // What follows on the lane starts after everything enqueued on the main stream so far AND (behind_accumulation) after the accumulation
    // of the commitment enqueued last: stream priorities do not keep a 8192-workgroup NTT pass from taking the CUs first (measured: the
    // pre-phase of the wire commitments took 2.1 ms instead of 0.35 behind it), so the start is placed by hand where the GPU has room — the
    // bucket reduction of that commitment, the point-wise kernels of the next round and the pre-phase of its commitment.
    int32_t start_behind_main(bool behind_accumulation) {
        if (!on) return PLK_OK;
        PLK_HIP(hipEventRecord(ctx->bg_go, ctx->stream));
        PLK_HIP(hipStreamWaitEvent(ctx->bg_stream, ctx->bg_go, 0));
        if (behind_accumulation && ctx->msm_enq != ctx->msm_fin) {
            plk_ctx::MsmSlot &L = ctx->slot[ctx->fifo[(ctx->msm_enq - 1) % plk_ctx::MSM_SLOTS]];
            if (L.acc_done) PLK_HIP(hipStreamWaitEvent(ctx->bg_stream, L.acc_done, 0));
        }
        return PLK_OK;
    }
    // the lane's work of this phase is all enqueued (marked where it ends, so that the main stream can be made to wait for it later) ...
    int32_t mark_done() { if (on) PLK_HIP(hipEventRecord(ctx->bg_done, ctx->bg_stream)); return PLK_OK; }
    // ... and the main stream waits for the mark
    int32_t main_waits() { if (on) PLK_HIP(hipStreamWaitEvent(ctx->stream, ctx->bg_done, 0)); return PLK_OK; }
};

// ---- what the rounds of one proof share: a round reads what the earlier ones left here and adds its own results
struct ProveState {
    plk_ctx *ctx;
    const plk_setup *S;
    const ProveWs &W;
    ProveFront &F;
    const uint64_t N;                        // the domain
    hipStream_t st;                          // the context's stream: the round-critical kernels
    BgLane lane;                             // (before the transcript: `end` runs first on the way out, then the lane is waited for)
    std::optional<ProofTranscript> tr;       // begins in round 1, once the front end's verdict is in; ends wherever the proof is left
    bool use_lagrange = false;               // the witness and grand-product polynomials are committed from their values (round 1 decides)
    HFr beta, gamma, alpha, v;
    ZPoint at;                               // the challenge z with its powers and inverses (round 4)
    HAffine wire_c[4], z_c, t_c[4], Wz, Wzw;
    Evals ev;
    PowTable pt_z, pt_zinv, pt_zw, pt_zwinv;
    void lap() { double t = now_ms(); ctx->timings.push_back(t - F.t_prev); F.t_prev = t; }
};
static void beta_k_dev(const HFr &beta, Fr out[4]) { for (int j = 0; j < 4; j++) out[j] = to_dev(beta * HFr::from_u64(NON_RESIDUES[j])); }

// ---- round 1: wire polynomials, 4 x iNTT(N) in one launch per pass, 4 x MSM(N)
static int32_t round1_wires(ProveState &P) {
    plk_ctx *ctx = P.ctx;
    const uint64_t N = P.N;
    PLK_TRY(ntt_columns_dev(ctx, P.W.w_coef, 4, P.S->log_n, true, P.st));
    // with a Lagrange-form key of the domain's size resident (`prove -l`, src/plonk.rs:138-146) the witness and
    // grand-product polynomials are committed from their evaluations, as bellman's prove() does; same proof bytes
    P.use_lagrange = ctx->lagrange().pts != nullptr;
    if (P.use_lagrange && (ctx->combine ? ctx->lagrange().n != ctx->srs().n : ctx->lagrange().n != N)) { set_error("Lagrange-form key has a different size than the circuit's domain"); return PLK_ERR_SRS; }
    PLK_TRY(commit_begin(ctx, P.use_lagrange ? P.W.w_vals : P.W.w_coef, 4, N, P.use_lagrange));
    // round-3 work that needs no challenge: the wire extensions start behind the wires' accumulation
    PLK_TRY(P.lane.start_behind_main(true));
    PLK_TRY(lde4cm_batch_dev(ctx, P.W.w_coef, 4, P.S->log_n, P.W.ext, P.lane.stream(), P.lane.ntt_lane()));
    PLK_HIP(hipEventSynchronize(ctx->flag_ready));
    PLK_TRY(front_verdict(ctx, P.S, P.F));
    PLK_TRY(commit_end(ctx, 4, P.wire_c));
    // the built-in Keccak transcript, or the table of plk_ctx_set_transcript: begin here, end wherever the function is left.  A
    // callback that failed or a challenge with limbs >= r ends the proof right behind the challenge, before anything consumes it
    P.tr.emplace(ctx->tr_set ? &ctx->tr_ops : nullptr, P.F.who);
    for (const HFr &x : P.F.inputs) P.tr->absorb_fr(x);
    for (int j = 0; j < 4; j++) P.tr->absorb_g1(P.wire_c[j]);
    P.beta = P.tr->challenge(); P.gamma = P.tr->challenge();
    return P.tr->report();
}

// The grand product z_i = prod_{k<i} num_k / den_k of a permutation argument, as values over the domain, without a per-element inversion:
// z_i = A_i * C_i / C_0 with A = exclusive prefix product of num, C = inclusive suffix product of den (pa.num, pa.den: scratch of n each).
// This is what round 2 runs between its challenges and the iNTT, and all of what plk_permutation_grand_product_dev runs.
// The scans stop after their second phase when they span several blocks: the block prefixes are folded in by the product (mul3_blocks),
// and C_0 — the product of all denominators — is the suffix scan's grand total, which its second phase leaves behind the prefixes.
// den_total <- C_0; num_total (optional) <- the product of all numerators, which sits in the scan's block-total slot (poly.hip: behind the
// nb prefixes; with one block the block total itself, lazily reduced) and comes back with the same synchronisation.
static int32_t grand_product(plk_ctx *ctx, const PermArgs &pa, Fr *out, hipStream_t st, const char *vanished, HFr *den_total, HFr *num_total) {
    PLK_TRY(perm_terms(pa, st));
    const Fr *pre_a = nullptr, *pre_c = nullptr;
    PLK_TRY(scan_pair_mult(ctx, pa.num, pa.num, false, true, pa.den, pa.den, true, false, pa.n, st, &pre_a, &pre_c));
    const uint32_t nb = (pa.n + POLY_SCAN_BLOCK - 1) / POLY_SCAN_BLOCK;
    PLK_HIP(hipMemcpyAsync(den_total->l, pre_c ? pre_c + nb : pa.den, sizeof(Fr), hipMemcpyDeviceToHost, st));
    if (num_total) PLK_HIP(hipMemcpyAsync(num_total->l, ctx->poly_tmp.as<Fr>() + (nb > 1 ? nb : 0), sizeof(Fr), hipMemcpyDeviceToHost, st));
    PLK_HIP(hipStreamSynchronize(st));
    if (den_total->is_zero()) { set_error(vanished); return PLK_ERR_UNSAT; }
    if (num_total && HFr::geq_p(num_total->l)) HFr::sub_p(num_total->l);
    // the scans live in the W domain: what was read is 32 * C_0, so E(1 / C_0) = 32 * E(1 / (32 C_0))
    const Fr inv_c0 = to_dev(to_w(den_total->inv()));
    if (pre_c) return mul3_blocks(out, pa.num, pa.den, pre_a, pre_c, inv_c0, pa.n, st);
    return mul3(out, pa.num, pa.den, inv_c0, pa.n, st);
}
static PermArgs perm_args(plk_ctx *ctx, const Fr *const w[4], const Fr *const sigma[4], const HFr &beta, const HFr &gamma, uint32_t log_n, Fr *num, Fr *den) {
    PermArgs pa;
    pa.num = num; pa.den = den;
    for (int j = 0; j < 4; j++) { pa.w[j] = w[j]; pa.sigma[j] = sigma[j]; }
    beta_k_dev(beta, pa.beta_k);
    pa.beta = to_dev(to_w(beta)); pa.gamma = to_dev(gamma); pa.fix = to_dev(HFr::from_u64(W_FOUR_E_FACTORS));
    pa.n = 1u << log_n; pa.log_n = log_n; pa.tw = ctx->tw_fwd_w;
    return pa;
}

// ---- round 2: grand product z
static int32_t round2_grand_product(ProveState &P) {
    plk_ctx *ctx = P.ctx;
    const plk_setup *S = P.S;
    hipStream_t st = P.st;
    const uint64_t N = P.N;
    HFr total, num_total;
    PLK_TRY(grand_product(ctx, perm_args(ctx, P.W.w_vals, S->sig_vals, P.beta, P.gamma, S->log_n, P.W.t1, P.W.t2), P.W.z_coef, st,
                          "grand product denominator vanished (probability ~2^-230)", &total, P.F.close_perm ? &num_total : nullptr));
    // copy constraints of a caller's sigma (assembled front): the argument closes iff prod num == prod den
    if (P.F.close_perm && num_total != total) {
        std::string msg = "copy constraints: the permutation argument does not close (prod of numerators != prod of denominators at beta, gamma): "
                          "the columns break the copy constraints of the setup's sigma";
        // which one: the exact checks on the columns as they sit in the workspace (only here, on the way out with an error)
        plk_copy_report rep;
        if (copy_check(ctx, S->sig_vals, S->log_n, P.W.w_vals, N, &rep, st) == PLK_OK) append_copy_report(msg, rep);
        set_error(msg);
        return PLK_ERR_UNSAT;
    }
    if (P.use_lagrange) PLK_HIP(hipMemcpyAsync(P.W.t1, P.W.z_coef, N * sizeof(Fr), hipMemcpyDeviceToDevice, st));   // keep the values
    PLK_TRY(ntt_dev(ctx, P.W.z_coef, S->log_n, true, nullptr, st));
    { const Fr *zp = P.use_lagrange ? P.W.t1 : P.W.z_coef; PLK_TRY(commit_begin(ctx, &zp, 1, N, P.use_lagrange)); }
    // while z is being committed: its extension and the public-input polynomial.  z's extension is the last thing the quotient waits for:
    // it starts behind the main stream only, as soon as z's coefficients exist, and shares the GPU with the accumulation of z's
    // commitment — behind that accumulation it ended 0.4 ms after the commitment itself
    PLK_TRY(P.lane.start_behind_main(false));
    hipStream_t bg = P.lane.stream();
    { const Fr *zc = P.W.z_coef; PLK_TRY(lde4cm_batch_dev(ctx, &zc, 1, S->log_n, &P.W.ext[4], bg, P.lane.ntt_lane())); }
    if (!P.W.direct_pi) {
        Fr *pi_coef = P.W.pi_coef;
        PLK_HIP(hipMemsetAsync(pi_coef, 0, N * sizeof(Fr), bg));
        PLK_HIP(hipMemcpyAsync(pi_coef, P.F.inputs.data(), P.F.inputs.size() * sizeof(Fr), hipMemcpyHostToDevice, bg));
        PLK_TRY(ntt_batch_dev(ctx, &pi_coef, 1, S->log_n, true, nullptr, bg, P.lane.ntt_lane()));
        const Fr *pc = pi_coef;
        PLK_TRY(lde4cm_batch_dev(ctx, &pc, 1, S->log_n, &P.W.ext[16], bg, P.lane.ntt_lane()));
    }
    PLK_TRY(P.lane.mark_done());
    PLK_TRY(commit_end(ctx, 1, &P.z_c));
    P.tr->absorb_g1(P.z_c);
    P.alpha = P.tr->challenge();
    return P.tr->report();
}

// The constants a setup's FIRST proof computes and every later one reads: the coset-major extensions of the 7 selectors, 4 sigmas and L_0
// (pre-scaled for the quotient kernel), the coset points, 1 / Z_H on the four cosets and the constants of the coset iNTT's combine step.
// One setup may be proved from several contexts / host threads at once: all of it under S->lazy_mu, complete on the device before
// lde_ready is set.
static int32_t setup_extensions_ready(plk_ctx *ctx, const plk_setup *S, const ProveWs &W, hipStream_t st) {
    const uint64_t N = S->N, M = 4 * N;
    const uint32_t log_n = S->log_n, log_m = log_n + 2;
    std::lock_guard<std::mutex> lazy_lock(S->lazy_mu);
    if (!S->lde_ready) {
        // the coset-point vector is a convenience (one load instead of two loads and two products per point):
        // above 2^24 gates its 4N * 32 bytes are better spent elsewhere (2^26 would not fit in 288 GB)
        static const bool no_cache_env = getenv("PLK_NO_COSET_CACHE") != nullptr;       // tests: the large-domain branch at a small size
        const int vectors = log_n <= 24 && !no_cache_env ? 13 : 12;
        PLK_TRY(S->lde_store.reserve(vectors * ((M * sizeof(Fr) + 255) & ~(size_t)255)));
        Arena LA{&S->lde_store};
        for (int k = 0; k < vectors; k++) S->lde[k] = LA.take<Fr>(M);
        if (vectors == 12) S->lde[12] = nullptr;
        HFr one = HFr::one();
        PLK_HIP(hipMemsetAsync(W.l0_coef, 0, N * sizeof(Fr), st));
        PLK_HIP(hipMemcpyAsync(W.l0_coef, one.l, sizeof(Fr), hipMemcpyHostToDevice, st));
        PLK_TRY(ntt_dev(ctx, W.l0_coef, log_n, true, nullptr, st));
        {   // 7 selectors, 4 sigmas, L0: twelve extensions in the coset-major layout of the quotient kernel, four polynomials per launch
            const Fr *src[12];
            for (int k = 0; k < 7; k++) src[k] = S->sel_coef[k];
            for (int j = 0; j < 4; j++) src[7 + j] = S->sig_coef[j];
            src[11] = W.l0_coef;
            PLK_TRY(lde4cm_batch_dev(ctx, src, 12, log_n, S->lde, st, 0));
        }
        // pre-scaled for the 29-bit layer of the quotient kernel (poly.h, QuotientArgs): 2^5 everywhere,
        // 2^10 on q_m, none on q_const (it is only added); plus the coset points x_i = 7 * omega_4N^i
        for (int k = 0; k < 12; k++) {
            if (k == 5) continue;
            PLK_TRY(scale_const(S->lde[k], S->lde[k], to_dev(HFr::from_u64(k == 4 ? W_LDE_SCALE_QM : W_LDE_SCALE)), (uint32_t)M, st));
        }
        if (S->lde[12]) PLK_TRY(coset_points_w(S->lde[12], ctx->tw_fwd_w, log_m, to_dev(HFr::from_u64(W_COSET_GEN)), (uint32_t)M, st));
        PLK_HIP(hipStreamSynchronize(st));
        S->lde_ready = true;
    }
    if (!S->zh_inv_ready) {                                   // 1 / Z_H on the four cosets of <omega_N> inside the 4N domain: circuit constants
        HFr gN = HFr::from_u64(7).pow_u64(N), iota = host_omega(2), ip = HFr::one();       // iota = omega_4N^N = omega_4
        for (int k = 0; k < 4; k++) { S->zh_inv[k] = (gN * ip - HFr::one()).inv(); ip = ip * iota; }
        icoset_constants(log_n, S->icoset_c);
        S->zh_inv_ready = true;
    }
    return PLK_OK;
}

// ---- round 3: quotient on the coset 7*<omega_4N>: 18 x LDE, fused point-wise kernel, coset iNTT(4N)
static int32_t round3_quotient(ProveState &P) {
    plk_ctx *ctx = P.ctx;
    const plk_setup *S = P.S;
    hipStream_t st = ctx->stream;
    const uint64_t N = S->N;
    PLK_TRY(setup_extensions_ready(ctx, S, P.W, st));
    QuotientArgs qa;
    qa.out = P.W.t_ext;
    for (int j = 0; j < 4; j++) { qa.w[j] = P.W.ext[j]; qa.sigma[j] = S->lde[7 + j]; }
    beta_k_dev(P.beta, qa.beta_k);
    qa.z = P.W.ext[4];
    for (int k = 0; k < 7; k++) qa.q[k] = S->lde[k];
    qa.pi = P.W.direct_pi ? nullptr : P.W.ext[16]; qa.l0 = S->lde[11]; qa.x = S->lde[12];
    qa.tw_w = ctx->tw_fwd_w; qa.coset_w = to_dev(HFr::from_u64(W_COSET_GEN));
    qa.num_pi = P.W.direct_pi ? (uint32_t)P.F.inputs.size() : 0;
    for (uint32_t k = 0; k < qa.num_pi; k++) qa.pi_in[k] = to_dev(P.F.inputs[k]);
    qa.beta = to_dev(P.beta); qa.gamma = to_dev(P.gamma);
    qa.alpha_pp = to_dev(P.alpha * HFr::from_u64(W_FOUR_E_FACTORS)); qa.alpha2_w = to_dev(to_w(P.alpha * P.alpha));
    for (int k = 0; k < 4; k++) qa.zh_inv_w[k] = to_dev(to_w(S->zh_inv[k]));
    qa.m = (uint32_t)(4 * N); qa.log_m = S->log_n + 2;
    PLK_TRY(P.lane.main_waits());                             // the five extensions (+ PI) of the background lane
    PLK_TRY(quotient(qa, st));
    // coset iNTT at 4N from the coset-major layout the kernel wrote: four inverse N-point coset transforms (one launch per
    // pass) and a 4-point combine, instead of three passes over 4N (0.57 -> 0.48 ms at the 2^20 domain)
    PLK_TRY(icoset4cm_dev(ctx, P.W.t_ext, S->log_n, st, 0));
    PLK_TRY(icoset_combine_ext(P.W.t_ext, (uint32_t)N, S->icoset_c, st));
    const Fr *parts[4] = {P.W.t_ext, P.W.t_ext + N, P.W.t_ext + 2 * N, P.W.t_ext + 3 * N};
    PLK_TRY(commit_many(ctx, parts, 4, N, P.t_c));
    P.lane.armed = false;                                     // the quotient consumed everything the background lane produced
    for (int k = 0; k < 4; k++) P.tr->absorb_g1(P.t_c[k]);
    P.at.z = P.tr->challenge();
    return P.tr->report();
}

// ---- round 4: evaluations at z and z*omega, linearisation
static int32_t round4_evaluations(ProveState &P) {
    plk_ctx *ctx = P.ctx;
    const plk_setup *S = P.S;
    hipStream_t st = ctx->stream;
    const uint32_t N = (uint32_t)S->N;
    if (const char *refused = challenge_point(HFr(P.at.z), host_omega(S->log_n), S->N, &P.at)) { set_error(refused); return PLK_ERR_UNSAT; }
    {
        const Fr bases4[4] = {to_dev(P.at.z), to_dev(P.at.z_inv), to_dev(P.at.zw), to_dev(P.at.zw_inv)};
        PowTable pts4[4];
        PLK_TRY(fill_pow_tables4_into(ctx, bases4, P.W.tab, pts4, st));
        P.pt_z = pts4[0]; P.pt_zinv = pts4[1]; P.pt_zw = pts4[2]; P.pt_zwinv = pts4[3];
    }
    {
        EvalArgs ea{};
        const Fr *polys[10] = {P.W.w_coef[0], P.W.w_coef[1], P.W.w_coef[2], P.W.w_coef[3], P.W.w_coef[3],
                               S->sig_coef[0], S->sig_coef[1], S->sig_coef[2], P.W.t_ext, P.W.z_coef};
        for (int e = 0; e < 10; e++) { ea.poly[e] = polys[e]; ea.len[e] = e == 8 ? 4 * N : N; ea.pt[e] = (e == 4 || e == 9) ? P.pt_zw : P.pt_z; }
        ea.count = 10;
        PLK_TRY(eval_batch(ctx, ea, P.W.d_results, st));
        PLK_HIP(hipMemcpyAsync(P.ev.v, P.W.d_results, 10 * sizeof(Fr), hipMemcpyDeviceToHost, st));
        PLK_HIP(hipStreamSynchronize(st));
    }
    {
        HFr fz, fs, sc[9];
        permutation_factors(P.alpha, P.beta, P.gamma, P.at, P.ev, &fz, &fs);
        linearisation_coefficients(P.ev, fz, fs, sc);
        LinCombArgs la{};
        la.out = P.W.r_poly; la.n = N; la.count = 9;
        const Fr *ps[9] = {S->sel_coef[5], S->sel_coef[0], S->sel_coef[1], S->sel_coef[2], S->sel_coef[3], S->sel_coef[4], S->sel_coef[6], P.W.z_coef, S->sig_coef[3]};
        for (int k = 0; k < 9; k++) { la.p[k] = ps[k]; la.s[k] = to_dev(to_w(sc[k])); la.unit[k] = (k == 0); }
        PLK_TRY(lincomb(la, st));
        EvalArgs ea{};
        ea.poly[0] = P.W.r_poly; ea.len[0] = N; ea.pt[0] = P.pt_z; ea.count = 1;
        PLK_TRY(eval_batch(ctx, ea, P.W.d_results, st));
        PLK_HIP(hipMemcpyAsync(&P.ev.v[10], P.W.d_results, sizeof(Fr), hipMemcpyDeviceToHost, st));
        PLK_HIP(hipStreamSynchronize(st));
    }
    for (int j = 0; j < 4; j++) P.tr->absorb_fr(P.ev.wz()[j]);
    P.tr->absorb_fr(P.ev.w3zw());
    for (int j = 0; j < 3; j++) P.tr->absorb_fr(P.ev.sz()[j]);
    P.tr->absorb_fr(P.ev.tz()); P.tr->absorb_fr(P.ev.rz()); P.tr->absorb_fr(P.ev.zzw());
    P.v = P.tr->challenge();
    return P.tr->report();
}

// (p(x) - p(z)) / (x - z) of a linear combination p = sum_k s_k p_k by synthetic division: q_k = z^-(k+1) * sum_{j > k} p_j z^j — the
// combination times z^i (la.times_pow = the table of z), suffix sums in place in la.out, times z^-(k+1) into out.  Round 5 runs it twice;
// plk_poly_divide_by_linear_dev runs it on one polynomial with the coefficient one.  totals: the scan's block totals (scan, poly.h).
static int32_t divide_by_linear(plk_ctx *ctx, const LinCombArgs &la, const PowTable &zinv, Fr *out, hipStream_t s, DevBuf *totals) {
    PLK_TRY(lincomb(la, s));
    PLK_TRY(scan(ctx, la.out, la.out, la.n, true, false, s, totals));
    return div_finish(out, la.out, zinv, la.n, s);
}

// ---- round 5: opening proofs W_z, W_zw
static int32_t round5_openings(ProveState &P) {
    plk_ctx *ctx = P.ctx;
    const plk_setup *S = P.S;
    const uint64_t N = S->N;
    Fr *const t_ext = P.W.t_ext;
    HFr at_z[12], at_zw[2];
    opening_coefficients(P.at.zN, P.v, at_z, at_zw);
    LinCombArgs la{};
    la.n = (uint32_t)N; la.count = 12;
    const Fr *ps[12] = {t_ext, t_ext + N, t_ext + 2 * N, t_ext + 3 * N, P.W.r_poly, P.W.w_coef[0], P.W.w_coef[1], P.W.w_coef[2], P.W.w_coef[3],
                        S->sig_coef[0], S->sig_coef[1], S->sig_coef[2]};
    for (int k = 0; k < 12; k++) { la.p[k] = ps[k]; la.s[k] = to_dev(to_w(at_z[k])); la.unit[k] = (k == 0); }
    la.times_pow = P.pt_z; la.out = P.W.t1;
    // The two quotients are independent chains of five small launches each (linear combination times z^i, suffix sums,
    // times z^-(k+1)): the second one runs on the background lane (idle since round 3) with scratch of its own, so that
    // the two chains overlap instead of queueing (0.14 ms of pure launch latency at the 2^20 domain).
    LinCombArgs lb{};
    lb.n = (uint32_t)N; lb.count = 2;
    lb.p[0] = P.W.z_coef; lb.s[0] = to_dev(to_w(at_zw[0])); lb.p[1] = P.W.w_coef[3]; lb.s[1] = to_dev(to_w(at_zw[1]));
    lb.times_pow = P.pt_zw;
    lb.out = P.lane.on ? P.W.pi_coef : P.W.t1;                    // (pi_coef: free since the quotient)
    P.lane.armed = P.lane.on;                                     // (an error below must not leave chain B writing into the arena)
    PLK_TRY(P.lane.start_behind_main(false));                     // the power tables and r(x) come from the main stream
    PLK_TRY(divide_by_linear(ctx, la, P.pt_zinv, P.W.t2, ctx->stream, nullptr));
    PLK_TRY(divide_by_linear(ctx, lb, P.pt_zwinv, P.W.t3, P.lane.stream(), P.lane.on ? &ctx->poly_tmp2 : nullptr));
    PLK_TRY(P.lane.mark_done());
    PLK_TRY(P.lane.main_waits());
    const Fr *opens[2] = {P.W.t2, P.W.t3};
    HAffine oc[2];
    PLK_TRY(commit_many(ctx, opens, 2, N, oc));
    P.lane.armed = false;                                         // the commitments consumed t3: chain B has ended
    P.Wz = oc[0]; P.Wzw = oc[1];
    return PLK_OK;
}

// ---- Proof::write, and what plk_prove_trace hands out (all of it lives in ctx->prove_ws until the next proof)
static int32_t write_proof(ProveState &P, uint8_t *proof_out, uint64_t cap, uint64_t *len) {
    const uint64_t N = P.S->N;
    const std::vector<HFr> &inputs = P.F.inputs;
    std::vector<uint8_t> b;
    put_u64(b, P.S->n);
    put_u64(b, inputs.size());
    for (const HFr &x : inputs) put_fr(b, x);
    put_u64(b, 4); for (int j = 0; j < 4; j++) put_g1(b, P.wire_c[j]);
    put_g1(b, P.z_c);
    put_u64(b, 4); for (int k = 0; k < 4; k++) put_g1(b, P.t_c[k]);
    put_u64(b, 4); for (int j = 0; j < 4; j++) put_fr(b, P.ev.wz()[j]);
    put_u64(b, 1); put_fr(b, P.ev.w3zw());
    put_fr(b, P.ev.zzw()); put_fr(b, P.ev.tz()); put_fr(b, P.ev.rz());
    put_u64(b, 3); for (int j = 0; j < 3; j++) put_fr(b, P.ev.sz()[j]);
    put_g1(b, P.Wz); put_g1(b, P.Wzw);
    *len = b.size();
    plk_ctx::Trace &t = P.ctx->trace;
    const Fr *vec[9] = {P.W.w_coef[0], P.W.w_coef[1], P.W.w_coef[2], P.W.w_coef[3], P.W.z_coef, P.W.t_ext, P.W.r_poly, P.W.t2, P.W.t3};
    for (int k = 0; k < 9; k++) { t.ptr[k] = vec[k]; t.len[k] = k == 5 ? 4 * N : N; }
    t.valid = true;
    if (b.size() > cap) { set_error("plk_prove: proof buffer too small"); return PLK_ERR_ARG; }
    memcpy(proof_out, b.data(), b.size());
    return PLK_OK;
}

// Rounds 1-5 and Proof::write, shared by plk_prove and plk_prove_assembled*: from the wire values a front end left in the workspace.
// Every step but the first ends with a plk_prove_timings entry ([0] is the front end's).
static int32_t prove_rounds(plk_ctx *ctx, const plk_setup *S, const ProveWs &W, ProveFront &F, uint8_t *proof_out, uint64_t cap, uint64_t *len) {
    ProveState P{ctx, S, W, F, S->N, ctx->stream};
    PLK_TRY(P.lane.open(ctx, S->log_n));
    PLK_TRY(round1_wires(P));             P.lap();        // [1] beta, gamma
    PLK_TRY(round2_grand_product(P));     P.lap();        // [2] alpha
    PLK_TRY(round3_quotient(P));          P.lap();        // [3] z
    PLK_TRY(round4_evaluations(P));       P.lap();        // [4] v
    PLK_TRY(round5_openings(P));          P.lap();        // [5]
    PLK_TRY(write_proof(P, proof_out, cap, len)); P.lap();    // [6] serialise
    return PLK_OK;
}

// Where the witness of a proof comes from: exactly one of the four is set.
struct WitnessSrc {
    const plk_circuit *c = nullptr;          // a circuit object: its witness vector, page-locked from the second proof of the object on
    const HFr *host = nullptr;               // n Montgomery elements in host memory (the caller's buffer: never page-locked)
    const Fr *dev = nullptr;                 // n Montgomery elements on the device, complete once the work enqueued on `caller` is
    const uint8_t *payload = nullptr;        // the n x 32 element bytes of a .wtns file whose container has been checked (wtnsio.hip decodes them)
    uint64_t n = 0;
    hipStream_t caller = nullptr;
    uint64_t *bad_out_of_file = nullptr;     // plk_prove_wtns: receives the lowest refused element of the file
};

// The witness front end of plk_prove* and plk_validate_witness*: the circom wires and the transpiler's temporaries, by variable id, in
// W->d_values on the device (enqueued on the context's stream).  whole_workspace: the arena of a proof (prove_workspace); otherwise only
// the values and the verdict words.  lap (may be empty) is called once, after the host part: [0] of plk_prove_timings.
// A witness that is not a circuit object's is checked on the device: the 64-bit word at W->d_flag + 2 receives the lowest wire in
// [1, num_variables) that is not a canonical residue (host and device vectors) or the lowest element of the file that is >= r (file
// bytes; every element of the file is looked at).  F (may be null): the public inputs, or where they are on their way to.
static int32_t witness_front(plk_ctx *ctx, const plk_setup *S, const WitnessSrc &src, const char *who, bool whole_workspace, ProveWs *W,
                             const std::function<void()> &lap, ProveFront *F) {
    hipStream_t st = ctx->stream;
    const plk_circuit *c = src.c;
    // ---- witness synthesis (host): circom wires, then the transpiler's temporaries from their recorded
    //      linear forms (the gate structure itself lives in plk_setup; the reference re-synthesises here)
    if (c ? (c->r1cs.num_variables != S->num_circuit_vars || c->witness.size() < S->num_circuit_vars) : src.n < S->num_circuit_vars) {
        set_error(std::string(who) + (c ? ": circuit does not match the prepared setup" : ": the witness does not match the prepared setup")); return PLK_ERR_ARG; }
    // circom wires are uploaded straight from the (page-locked) witness buffer; only the temporaries are
    // computed here, into a pinned staging area.  id 0 (dummy) is zeroed on the device.
    const uint64_t ncv = S->num_circuit_vars, n_tmp = S->num_vars - ncv;
    // page-locking the witness (hipHostRegister) makes its upload 2 ms faster at 2^20 but costs ~50 ms once, plus the
    // un-pinning when the process ends: worth it from the second proof of the same circuit object on, not for the
    // one-proof-per-process pattern of the CLI (profiles/r02_cli_scale.txt: 0.36 -> 0.29 s whole `plonkit prove`)
    static const int reg_mode = [] { const char *e = getenv("PLK_HOST_REGISTER"); return !e ? 1 : (!strcmp(e, "always") ? 0 : (!strcmp(e, "never") ? 1 << 30 : 1)); }();
    // Only a witness that owns its pages is page-locked: >= 4 MB sits in a 2 MiB-aligned block of its own (circuit.h, HugeAlloc).
    // A small one lives on the malloc heap and shares its 4 KiB pages with unrelated objects — numpy buffers, other circuits'
    // witnesses — that the runtime locks and unlocks on its own for pageable copies; pinning and unpinning such pages behind its
    // back ended, once in two or three runs of the whole GPU test suite, in "Memory access fault by GPU ... on address <heap page>"
    // during a LATER, unrelated host-to-device copy (round 4; profiles/r04_host_register_fault.txt).  A small upload gains nothing anyway.
    // A caller's own vector (plk_prove_witness) is never page-locked, whatever its size.
    if (c) {
        std::lock_guard<std::mutex> reg_lock(c->reg_mu);
        const size_t wit_bytes = c->witness.size() * sizeof(HFr);
        if (!c->witness_registered && wit_bytes >= ((size_t)4 << 20) && (int)(c->proofs_started++) >= reg_mode) {
            if (hipHostRegister((void *)c->witness.data(), wit_bytes, hipHostRegisterDefault) == hipSuccess) c->witness_registered = true;
            else (void)hipGetLastError();                                    // not fatal: the copy is just slower
        }
    }
    static const bool tmp_host_env = [] { const char *e = getenv("PLK_WITNESS_TMP_HOST"); return e && e[0] == '1'; }();      // tests: the host loop
    const bool tmp_on_device = !tmp_host_env && (S->ops_independent || S->ops_chained) && (S->ops_dev.p || S->ops.empty());
    const HFr *wit = c ? c->witness.data() : src.host;                         // null: the witness is on the device, or still file bytes
    const bool inputs_from_device = !wit && tmp_on_device && F && S->num_inputs;
    PLK_TRY(ensure_pinned2(ctx, (tmp_on_device ? (inputs_from_device ? S->num_inputs : 1) : n_tmp + 1) * sizeof(HFr)));
    HFr *tmp_vals = reinterpret_cast<HFr *>(ctx->pinned2);
    auto host_temporaries = [&](const HFr *w) {
        const size_t n_ops = S->ops.size();
        auto value_of = [&](uint32_t v) -> HFr { return v == 0 ? HFr::zero() : (v < ncv ? w[v] : tmp_vals[v - ncv]); };
        auto eval_range = [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                const WitnessOp &op = S->ops[i];
                HFr acc = op.constant;
                for (uint32_t k = 0; k < op.count; k++) { const WitnessTerm &t = S->op_terms[op.first + k]; acc = acc + t.coeff * value_of(t.var); }
                tmp_vals[i] = acc;
            }
        };
        if (S->ops_independent && n_ops > 4096) {
            unsigned nt = std::thread::hardware_concurrency();
            if (nt > 16) nt = 16;
            if (nt < 1) nt = 1;
            std::vector<std::thread> th;
            size_t per = (n_ops + nt - 1) / nt;
            for (unsigned t = 0; t < nt; t++) { size_t lo = t * per, hi = std::min(n_ops, lo + per); if (lo < hi) th.emplace_back(eval_range, lo, hi); }
            for (auto &x : th) x.join();
        } else eval_range(0, n_ops);
    };
    auto workspace = [&]() -> int32_t {
        if (whole_workspace) return prove_workspace(ctx, S, S->num_vars, W);
        // plk_validate_witness*: the values and the verdict words only
        PLK_TRY(ctx->prove_ws.reserve(((S->num_vars * sizeof(Fr) + 255) & ~(size_t)255) + 256));
        Arena A{&ctx->prove_ws};
        W->d_values = A.take<Fr>(S->num_vars);
        W->d_flag = A.take<uint32_t>(64);
        return PLK_OK;
    };
    if (wit) {
        if (!tmp_on_device) host_temporaries(wit);
        if (lap) lap();                                                       // [0] witness synthesis
        PLK_TRY(workspace());
        if (c) {   // (under the circuit's lock: another context proving the SAME circuit object may be about to page-lock this buffer —
                   //  not while a pageable copy of it is being staged)
            std::lock_guard<std::mutex> upload_lock(c->reg_mu);
            PLK_HIP(hipMemcpyAsync(W->d_values, wit, ncv * sizeof(Fr), hipMemcpyHostToDevice, st));
        } else PLK_HIP(hipMemcpyAsync(W->d_values, wit, ncv * sizeof(Fr), hipMemcpyHostToDevice, st));       // pageable
        if (F) F->inputs.assign(wit + 1, wit + 1 + S->num_inputs);
    } else {
        PLK_TRY(workspace());
        unsigned long long *d_wire = reinterpret_cast<unsigned long long *>(W->d_flag + 2);
        PLK_HIP(hipMemsetAsync(d_wire, 0xff, 8, st));
        if (src.dev) {
            if (src.caller && src.caller != st) {                             // ordered after what the caller has enqueued on its stream
                if (!ctx->in_ready) PLK_HIP(hipEventCreateWithFlags(&ctx->in_ready, hipEventDisableTiming));
                PLK_HIP(hipEventRecord(ctx->in_ready, src.caller));
                PLK_HIP(hipStreamWaitEvent(st, ctx->in_ready, 0));
            }
            PLK_HIP(hipMemcpyAsync(W->d_values, src.dev, ncv * sizeof(Fr), hipMemcpyDeviceToDevice, st));
        } else PLK_TRY(wtns_payload_to_dev(ctx, src.payload, src.n, W->d_values, ncv, d_wire, st));
    }
    Fr *const d_values = W->d_values;
    if (!c && !src.payload) {                                                 // (a file's elements have been range-checked by the decode kernel)
        unsigned long long *d_wire = reinterpret_cast<unsigned long long *>(W->d_flag + 2);
        if (wit) PLK_HIP(hipMemsetAsync(d_wire, 0xff, 8, st));
        PLK_TRY(fr_canonical_launch(d_values, 1, ncv, d_wire, st));
    }
    PLK_HIP(hipMemsetAsync(d_values, 0, sizeof(Fr), st));
    std::vector<HFr> back;
    if (!wit) {
        if (!tmp_on_device) {   // a setup whose temporaries need the host loop: the wires come back once
            back.resize(ncv);
            PLK_HIP(hipMemcpyAsync(back.data(), d_values, ncv * sizeof(Fr), hipMemcpyDeviceToHost, st));
            PLK_HIP(hipStreamSynchronize(st));
            host_temporaries(back.data());
            if (F) F->inputs.assign(back.data() + 1, back.data() + 1 + S->num_inputs);
        } else if (inputs_from_device) {                                      // the few public inputs travel behind the verdict's event
            PLK_HIP(hipMemcpyAsync(ctx->pinned2, d_values + 1, S->num_inputs * sizeof(Fr), hipMemcpyDeviceToHost, st));
            F->inputs_pinned = reinterpret_cast<const HFr *>(ctx->pinned2);
        }
        if (lap) lap();                                                       // [0] witness ingest
    }
    if (n_tmp && tmp_on_device && S->ops_chained)
        PLK_TRY(eval_witness_runs(d_values, S->ops_dev.p, S->terms_dev.p, S->runs_dev.p, (uint32_t)S->run_start.size(), (uint32_t)S->ops.size(), (uint32_t)ncv, st));
    else if (n_tmp && tmp_on_device) PLK_TRY(eval_witness_ops(d_values, S->ops_dev.p, S->terms_dev.p, (uint32_t)S->ops.size(), (uint32_t)ncv, st));
    else if (n_tmp) PLK_HIP(hipMemcpyAsync(d_values + ncv, tmp_vals, n_tmp * sizeof(Fr), hipMemcpyHostToDevice, st));
    return PLK_OK;
}


// `who`: plk_prove (a circuit object) or one of plk_prove_witness / _witness_dev / _wtns (src.c null)
static int32_t prove_impl(plk_ctx *ctx, const plk_setup *S, const WitnessSrc &src, const char *who, uint8_t *proof_out, uint64_t cap, uint64_t *len) {
    const plk_circuit *c = src.c;
    *len = 0;
    if (S->from_polys) {
        set_error(std::string(who) + ": this setup was built from polynomials (plk_setup_from_polynomials) and has no gate structure: "
                  "prove it from assembled columns with plk_prove_assembled / plk_prove_assembled_dev");
        return PLK_ERR_ARG;
    }
    if (c && !c->has_witness) { set_error("plk_prove: circuit has no witness"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    if (!ctx->srs().pts || (!ctx->combine && ctx->srs().n < S->N)) { set_error("SRS too small for this circuit"); return PLK_ERR_SRS; }
    if (!S->store.p) { set_error(std::string(who) + ": the setup is not on the device yet (plk_setup_upload)"); return PLK_ERR_ARG; }
    PLK_TRY(fifo_must_be_empty(ctx, who));
    FifoGuard fifo_guard(ctx);
    ctx->timings.clear();
    ctx->trace.valid = false;
    double t_prev = now_ms();
    auto lap = [&]() { double t = now_ms(); ctx->timings.push_back(t - t_prev); t_prev = t; };
    hipStream_t st = ctx->stream;

    ProveWs W;
    ProveFront F;
    F.who = who;
    F.wire_check = c ? 0 : (src.payload ? 2 : 1);
    PLK_TRY(witness_front(ctx, S, src, who, true, &W, lap, &F));
    const uint64_t N = S->N;
    Fr *const d_values = W.d_values;
    uint32_t *const d_flag = W.d_flag;
    {   // is_satisfied_using_one_shot_check (src/plonk.rs:137) on the device
        CheckArgs ca;
        ca.values = d_values; ca.n = (uint32_t)N; ca.num_inputs = (uint32_t)S->num_inputs; ca.flag = d_flag;
        for (int k = 0; k < 7; k++) ca.q[k] = S->sel_vals[k];
        for (int j = 0; j < 4; j++) ca.vars[j] = S->gate_vars[j];
        PLK_HIP(hipMemsetAsync(d_flag, 0, 4, st));
        PLK_TRY(check_gates(ca, st));
        // the verdict is read back into the pinned result buffer and looked at after round 1 has been enqueued (before any
        // commitment is used): the host does not stall the GPU for it.  An unsatisfied witness still ends the call with
        // PLK_ERR_UNSAT and no proof bytes — the commitments under way are drained by the FIFO guard.
        // (with a witness that was checked on the device, the word of that check travels with it: bytes 8..16)
        PLK_HIP(hipMemcpyAsync(ctx->pinned, d_flag, F.wire_check ? 16 : 4, hipMemcpyDeviceToHost, st));
        if (!ctx->flag_ready) PLK_HIP(hipEventCreateWithFlags(&ctx->flag_ready, hipEventDisableTiming));
        PLK_HIP(hipEventRecord(ctx->flag_ready, st));
    }
    PLK_TRY(gather4_dual(W.w_vals, W.w_coef, d_values, S->gate_vars, (uint32_t)N, st));
    F.t_prev = t_prev;
    const int32_t rc = prove_rounds(ctx, S, W, F, proof_out, cap, len);
    if (src.bad_out_of_file) *src.bad_out_of_file = F.wire_bad;
    return rc;
}

// SetupForProver::validate_witness (src/plonk.rs:127-129): the witness front end of plk_prove and the gate equation of every row, on their
// own — no key, no commitment, no round.  The verdict names the lowest failing row (the row kernel of the assembled path, assembled.hip,
// reports the same way; here it is an atomicMin on a 64-bit word).
static int32_t validate_witness_impl(plk_ctx *ctx, const plk_setup *S, const WitnessSrc &src, const char *who, int32_t *valid, uint64_t *bad_row) {
    const plk_circuit *c = src.c;
    if (S->from_polys) {
        set_error(std::string(who) + ": this setup was built from polynomials (plk_setup_from_polynomials) and has no gate structure: "
                  "the assembled columns are checked by plk_prove_assembled / plk_prove_assembled_dev");
        return PLK_ERR_ARG;
    }
    if (c && !c->has_witness) { set_error("plk_validate_witness: circuit has no witness"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    if (!S->store.p) { set_error(std::string(who) + ": the setup is not on the device yet (plk_setup_upload)"); return PLK_ERR_ARG; }
    PLK_TRY(fifo_must_be_empty(ctx, who));
    ctx->trace.valid = false;                                                 // the workspace the trace points into is written below
    hipStream_t st = ctx->stream;
    ProveWs W;
    PLK_TRY(witness_front(ctx, S, src, who, false, &W, nullptr, nullptr));
    unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(W.d_flag);
    CheckArgs ca;
    ca.values = W.d_values; ca.n = (uint32_t)S->N; ca.num_inputs = (uint32_t)S->num_inputs; ca.flag = nullptr;
    for (int k = 0; k < 7; k++) ca.q[k] = S->sel_vals[k];
    for (int j = 0; j < 4; j++) ca.vars[j] = S->gate_vars[j];
    PLK_HIP(hipMemsetAsync(d_bad, 0xff, 8, st));
    PLK_TRY(check_gates_row(ca, d_bad, st));
    unsigned long long got[2] = {~0ull, ~0ull};
    PLK_HIP(hipMemcpyAsync(got, d_bad, c ? 8 : 16, hipMemcpyDeviceToHost, st));
    PLK_HIP(hipStreamSynchronize(st));                                        // the verdict is this call's return value
    if (got[1] != ~0ull) {
        set_error(std::string(who) + ": wire " + std::to_string(got[1]) + " holds an element that is not a canonical residue (limbs >= r)");
        return PLK_ERR_ARG;
    }
    *valid = got[0] == ~0ull ? 1 : 0;
    if (bad_row) *bad_row = got[0];
    return PLK_OK;
}

// argument checks of the entry points that take a witness without its circuit, then the shared implementation
static int32_t prove_witness_entry(plk_ctx *ctx, const plk_setup *S, WitnessSrc src, const char *who, uint8_t *proof_out, uint64_t cap, uint64_t *len) {
    if (len) *len = 0;
    if (!ctx || !S || !proof_out || !len || (!src.host && !src.dev && !src.payload)) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    if (src.dev && ((uintptr_t)src.dev & 15u)) { set_error(std::string(who) + ": the witness must be 16-byte aligned"); return PLK_ERR_ARG; }
    return prove_impl(ctx, S, src, who, proof_out, cap, len);
}

// ---- the assembled-input path: SetupPolynomials (src/plonk.rs:50-55,104) and prove_by_steps on a circuit bellman has synthesised
//      (src/plonk.rs:152-159) — the setup polynomials and the four wire columns come from the caller, not from this library's transpiler
static int32_t setup_polys_impl(plk_ctx *ctx, uint64_t n, uint64_t num_inputs, const plk_fr *const selectors[6], const plk_fr *next_step,
                                const plk_fr *const sigmas[4], uint64_t len, uint32_t flags, plk_setup **out) {
    if (!ctx || !selectors || !next_step || !sigmas || !out) { set_error("plk_setup_from_polynomials: bad argument"); return PLK_ERR_ARG; }
    *out = nullptr;
    const plk_fr *src[11];
    for (int k = 0; k < 6; k++) src[k] = selectors[k];
    src[6] = next_step;
    for (int j = 0; j < 4; j++) src[7 + j] = sigmas[j];
    for (int i = 0; i < 11; i++) if (!src[i]) { set_error("plk_setup_from_polynomials: a selector or sigma vector is NULL"); return PLK_ERR_ARG; }
    if (flags & ~PLK_POLY_VALUES) { set_error("plk_setup_from_polynomials: unknown flag bits"); return PLK_ERR_ARG; }
    const uint64_t N = n + 1;
    if (N < 2 || (N & (N - 1))) { set_error("setup power of two is not in the correct range (n + 1 must be a power of two)"); return PLK_ERR_SIZE; }
    uint32_t log_n = 0;
    while ((1ull << log_n) < N) log_n++;
    if (log_n + 2 > MAX_LOG_N) { set_error("setup power of two is not in the correct range"); return PLK_ERR_SIZE; }   // src/plonk.rs:109-112
    const bool values = (flags & PLK_POLY_VALUES) != 0;
    if (values ? len != N : (len == 0 || len > N)) {
        set_error(values ? "plk_setup_from_polynomials: value form needs len == N = n + 1 evaluations per vector"
                         : "plk_setup_from_polynomials: coefficient form needs 1 <= len <= N = n + 1");
        return PLK_ERR_ARG;
    }
    if (num_inputs > n) { set_error("plk_setup_from_polynomials: num_inputs exceeds n"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<plk_setup, void (*)(plk_setup *)> S(new plk_setup(), plk_setup_free);
    S->n = n; S->N = N; S->log_n = log_n; S->num_inputs = num_inputs; S->n_real = n;
    S->from_polys = true;
    hipStream_t st = ctx->stream;
    // no variable-index columns, no permutation sort, no witness records: 22 vectors of N (the circuit path adds 4 x N x 4 B of indices)
    PLK_TRY(S->store.reserve(22 * ((N * sizeof(Fr) + 255) & ~(size_t)255) + 256));
    Arena A{&S->store};
    for (int k = 0; k < 7; k++) S->sel_coef[k] = A.take<Fr>(N);
    for (int k = 0; k < 7; k++) S->sel_vals[k] = A.take<Fr>(N);
    for (int j = 0; j < 4; j++) S->sig_coef[j] = A.take<Fr>(N);
    for (int j = 0; j < 4; j++) S->sig_vals[j] = A.take<Fr>(N);
    uint32_t *flag = A.take<uint32_t>(64);
    // given form -> the other one: coefficients get one forward NTT each (the values the gate check and round 2 read), values one iNTT each
    Fr *given[11], *derived[11];
    for (int k = 0; k < 7; k++) { given[k] = values ? S->sel_vals[k] : S->sel_coef[k]; derived[k] = values ? S->sel_coef[k] : S->sel_vals[k]; }
    for (int j = 0; j < 4; j++) { given[7 + j] = values ? S->sig_vals[j] : S->sig_coef[j]; derived[7 + j] = values ? S->sig_coef[j] : S->sig_vals[j]; }
    PLK_HIP(hipMemsetAsync(flag, 0, 4, st));
    for (int i = 0; i < 11; i++) {                               // pageable copies: the caller's buffers are not page-locked
        PLK_HIP(hipMemcpyAsync(given[i], src[i], len * sizeof(Fr), hipMemcpyHostToDevice, st));
        if (len < N) PLK_HIP(hipMemsetAsync(given[i] + len, 0, (N - len) * sizeof(Fr), st));
    }
    PLK_TRY(check_canonical(given, 11, len, flag, st));
    for (int i = 0; i < 11; i++) PLK_HIP(hipMemcpyAsync(derived[i], given[i], N * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    // (four transforms per launch where the batch scratch is small, one at a time above, as the circuit path's setup does)
    PLK_TRY(ntt_columns_dev(ctx, derived, 11, log_n, values, st));
    uint32_t bad = 0;
    PLK_HIP(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st));
    PLK_HIP(hipStreamSynchronize(st));
    if (bad) {
        static const char *const names[11] = {"q_a", "q_b", "q_c", "q_d", "q_m", "q_const", "q_d_next", "sigma_1", "sigma_2", "sigma_3", "sigma_4"};
        std::string which;
        for (int i = 0; i < 11; i++) if (bad >> i & 1) { which += which.empty() ? "" : ", "; which += names[i]; }
        set_error("plk_setup_from_polynomials: " + which + " holds an element that is not a canonical residue (limbs >= r)");
        return PLK_ERR_ARG;
    }
    *out = S.release();
    return PLK_OK;
}

// the assembled front end: columns a, b, c, d (rows values each, zero beyond) -> w_vals / w_coef, gate check, public inputs = a[0, num_inputs)
static int32_t prove_assembled_impl(plk_ctx *ctx, const plk_setup *S, const void *const cols[4], bool on_device, uint64_t rows,
                                    uint8_t *proof_out, uint64_t cap, uint64_t *len, hipStream_t caller) {
    const std::string who = on_device ? "plk_prove_assembled_dev" : "plk_prove_assembled";
    if (!ctx || !S || !cols || !proof_out || !len) { set_error(who + ": bad argument"); return PLK_ERR_ARG; }
    *len = 0;
    for (int j = 0; j < 4; j++) if (!cols[j]) { set_error(who + ": a column pointer is NULL"); return PLK_ERR_ARG; }
    if (rows < S->num_inputs || rows > S->N) { set_error(who + ": rows must satisfy num_inputs <= rows <= N"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    if (!ctx->srs().pts || (!ctx->combine && ctx->srs().n < S->N)) { set_error("SRS too small for this circuit"); return PLK_ERR_SRS; }
    if (!S->store.p) { set_error(who + ": the setup is not on the device yet (plk_setup_upload)"); return PLK_ERR_ARG; }
    PLK_TRY(fifo_must_be_empty(ctx, who.c_str()));
    FifoGuard fifo_guard(ctx);
    ctx->timings.clear();
    ctx->trace.valid = false;
    ProveFront F;
    F.who = on_device ? "plk_prove_assembled_dev" : "plk_prove_assembled";
    F.assembled = true;
    F.close_perm = true;
    F.t_prev = now_ms();
    hipStream_t st = ctx->stream;
    const uint64_t N = S->N;
    ProveWs W;
    PLK_TRY(prove_workspace(ctx, S, 0, &W));
    IngestArgs ia;
    if (on_device) {
        if (caller && caller != st) {                             // ordered after what the caller has enqueued on its stream
            if (!ctx->in_ready) PLK_HIP(hipEventCreateWithFlags(&ctx->in_ready, hipEventDisableTiming));
            PLK_HIP(hipEventRecord(ctx->in_ready, caller));
            PLK_HIP(hipStreamWaitEvent(st, ctx->in_ready, 0));
        }
        for (int j = 0; j < 4; j++) ia.src[j] = static_cast<const Fr *>(cols[j]);
    } else {
        // pageable copies into the quotient's 4N scratch (free until round 3): the caller's buffers are never page-locked (see the
        // witness note in prove_impl — pinning heap pages behind the runtime's back once ended in a GPU memory fault)
        for (int j = 0; j < 4; j++) {
            if (rows) PLK_HIP(hipMemcpyAsync(W.t_ext + j * N, cols[j], rows * sizeof(Fr), hipMemcpyHostToDevice, st));
            ia.src[j] = W.t_ext + j * N;
        }
        const HFr *a = static_cast<const HFr *>(cols[0]);
        F.inputs.assign(a, a + S->num_inputs);
    }
    { double t = now_ms(); ctx->timings.push_back(t - F.t_prev); F.t_prev = t; }     // [0] column upload
    for (int k = 0; k < 7; k++) ia.q[k] = S->sel_vals[k];
    for (int j = 0; j < 4; j++) { ia.vals[j] = W.w_vals[j]; ia.coef[j] = W.w_coef[j]; }
    ia.n = (uint32_t)N; ia.rows = (uint32_t)rows; ia.num_inputs = (uint32_t)S->num_inputs; ia.flag = W.d_flag;
    PLK_HIP(hipMemsetAsync(W.d_flag, 0, 8, st));
    PLK_TRY(ingest_columns(ia, st));
    // the verdict (and the public inputs of device columns) travel behind the same event as the circuit path's verdict: read after round 1
    // has been enqueued, no extra stall
    PLK_HIP(hipMemcpyAsync(ctx->pinned, W.d_flag, 8, hipMemcpyDeviceToHost, st));
    if (on_device && S->num_inputs) {
        PLK_TRY(ensure_pinned2(ctx, S->num_inputs * sizeof(HFr)));
        PLK_HIP(hipMemcpyAsync(ctx->pinned2, W.w_vals[0], S->num_inputs * sizeof(Fr), hipMemcpyDeviceToHost, st));
        F.inputs_pinned = reinterpret_cast<const HFr *>(ctx->pinned2);
    }
    if (!ctx->flag_ready) PLK_HIP(hipEventCreateWithFlags(&ctx->flag_ready, hipEventDisableTiming));
    PLK_HIP(hipEventRecord(ctx->flag_ready, st));
    return prove_rounds(ctx, S, W, F, proof_out, cap, len);
}

// ---- which copy constraint is broken (copycheck.hip): the setup's resident sigma values, and a caller's columns under the rules of
//      plk_prove_assembled* (num_inputs <= rows <= N, zero beyond rows, every element canonical)
static int32_t check_copies_impl(plk_ctx *ctx, const plk_setup *S, const void *const cols[4], bool with_cols, bool on_device, uint64_t rows, plk_copy_report *out,
                                 hipStream_t caller, const char *who_c) {
    const std::string who = who_c;
    if (out) *out = plk_copy_report{PLK_COPY_OK, 0, 0, 0, 0};
    if (!ctx || !S || !out || (with_cols && !cols)) { set_error(who + ": bad argument"); return PLK_ERR_ARG; }
    for (int j = 0; with_cols && j < 4; j++) if (!cols[j]) { set_error(who + ": a column pointer is NULL"); return PLK_ERR_ARG; }
    if (with_cols && (rows < S->num_inputs || rows > S->N)) { set_error(who + ": rows must satisfy num_inputs <= rows <= N"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    if (!S->store.p) { set_error(who + ": the setup is not on the device yet (plk_setup_upload)"); return PLK_ERR_ARG; }
    hipStream_t st = caller ? caller : ctx->stream;
    if (!with_cols) return copy_check(ctx, S->sig_vals, S->log_n, nullptr, 0, out, st);
    DevBuf tmp;                                                   // the canonicity flag, then (host columns) the four uploads
    const size_t CB = (rows * sizeof(Fr) + 255) & ~(size_t)255;
    PLK_TRY(tmp.reserve(256 + (on_device ? 0 : 4 * CB)));
    uint32_t *flag = tmp.as<uint32_t>();
    const Fr *src[4];
    int32_t rc = PLK_OK;
    uint32_t bad = 0;
    if (hipMemsetAsync(flag, 0, 4, st) != hipSuccess) rc = hip_fail(hipGetLastError(), "memset", __FILE__, __LINE__);
    for (int j = 0; j < 4; j++) {
        if (on_device) { src[j] = static_cast<const Fr *>(cols[j]); continue; }
        Fr *d = reinterpret_cast<Fr *>((char *)tmp.p + 256 + j * CB);
        if (rc == PLK_OK && rows && hipMemcpyAsync(d, cols[j], rows * sizeof(Fr), hipMemcpyHostToDevice, st) != hipSuccess) rc = hip_fail(hipGetLastError(), "H2D columns", __FILE__, __LINE__);
        src[j] = d;
    }
    if (rc == PLK_OK) rc = check_canonical(src, 4, rows, flag, st);
    if (rc == PLK_OK && hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st) != hipSuccess) rc = hip_fail(hipGetLastError(), "D2H", __FILE__, __LINE__);
    if (rc == PLK_OK) rc = copy_check(ctx, S->sig_vals, S->log_n, src, rows, out, st);      // (synchronises st: `bad` has arrived)
    else (void)hipStreamSynchronize(st);
    tmp.release();
    if (rc == PLK_OK && bad) {
        std::string which;
        for (int j = 0; j < 4; j++) if (bad >> j & 1) { which += which.empty() ? "" : ", "; which += "abcd"[j]; }
        set_error(who + ": column " + which + " holds an element that is not a canonical residue (limbs >= r)");
        *out = plk_copy_report{PLK_COPY_OK, 0, 0, 0, 0};
        return PLK_ERR_ARG;
    }
    return rc;
}

// ---- tracing / test hooks: the vectors between the rounds, and the polynomial helpers of rounds 2, 4 and 5 on their own
int32_t plk_prove_trace(plk_ctx *ctx, uint32_t which, plk_fr *out_host, uint64_t cap, uint64_t *n) {
    if (!ctx || !n || which >= 9) { set_error("plk_prove_trace: bad argument"); return PLK_ERR_ARG; }
    if (!ctx->trace.valid) { set_error("plk_prove_trace: no finished plk_prove on this context"); return PLK_ERR_ARG; }
    *n = ctx->trace.len[which];
    if (!out_host) return PLK_OK;
    if (cap < *n) { set_error("plk_prove_trace: buffer too small"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    PLK_HIP(hipMemcpyAsync(out_host, ctx->trace.ptr[which], *n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    PLK_HIP(hipStreamSynchronize(ctx->stream));
    return PLK_OK;
}

int32_t plk_poly_evaluate_at_dev(plk_ctx *ctx, const void *coeffs_dev, uint64_t n, const plk_fr *z, plk_fr *out, void *stream) {
    if (!ctx || !coeffs_dev || !z || !out || n == 0 || n > (1ull << MAX_LOG_N)) { set_error("plk_poly_evaluate_at_dev: bad argument"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    DevBuf tab;
    int32_t rc = tab.reserve((size_t)2 * POW_TAB * sizeof(Fr) + 64);
    if (rc != PLK_OK) return rc;
    Fr zz; memcpy(zz.l, z->l, 32);
    PowTable pt;
    rc = fill_pow_table_into(ctx, zz, tab.as<Fr>(), &pt, st);
    EvalArgs ea{};
    ea.poly[0] = (const Fr *)coeffs_dev; ea.len[0] = (uint32_t)n; ea.pt[0] = pt; ea.count = 1;
    Fr *res = tab.as<Fr>() + 2 * POW_TAB;
    if (rc == PLK_OK) rc = eval_batch(ctx, ea, res, st);
    if (rc == PLK_OK && hipMemcpyAsync(out, res, sizeof(Fr), hipMemcpyDeviceToHost, st) != hipSuccess) rc = hip_fail(hipGetLastError(), "D2H", __FILE__, __LINE__);
    if (hipStreamSynchronize(st) != hipSuccess && rc == PLK_OK) rc = hip_fail(hipGetLastError(), "sync", __FILE__, __LINE__);
    tab.release();
    return rc;
}

int32_t plk_poly_divide_by_linear_dev(plk_ctx *ctx, const void *coeffs_dev, uint64_t n, const plk_fr *z, void *quotient_dev, void *stream) {
    if (!ctx || !coeffs_dev || !z || !quotient_dev || n == 0 || n > (1ull << MAX_LOG_N)) { set_error("plk_poly_divide_by_linear_dev: bad argument"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    HFr hz; memcpy(hz.l, z->l, 32);
    if (hz.is_zero()) { set_error("plk_poly_divide_by_linear_dev: z = 0"); return PLK_ERR_ARG; }
    DevBuf tab;
    int32_t rc = tab.reserve((size_t)4 * POW_TAB * sizeof(Fr) + (size_t)n * sizeof(Fr));
    if (rc != PLK_OK) return rc;
    PowTable pzi;
    LinCombArgs la{};                                             // round 5's chain on the one polynomial, coefficient one
    la.out = tab.as<Fr>() + 4 * POW_TAB; la.n = (uint32_t)n; la.count = 1;
    la.p[0] = (const Fr *)coeffs_dev; la.unit[0] = 1;
    rc = fill_pow_table_into(ctx, to_dev(hz), tab.as<Fr>(), &la.times_pow, st);
    if (rc == PLK_OK) rc = fill_pow_table_into(ctx, to_dev(hz.inv()), tab.as<Fr>() + 2 * POW_TAB, &pzi, st);
    if (rc == PLK_OK) rc = divide_by_linear(ctx, la, pzi, (Fr *)quotient_dev, st, nullptr);
    if (hipStreamSynchronize(st) != hipSuccess && rc == PLK_OK) rc = hip_fail(hipGetLastError(), "sync", __FILE__, __LINE__);
    tab.release();
    return rc;
}

int32_t plk_permutation_grand_product_dev(plk_ctx *ctx, const void *const wires_dev[4], const void *const sigmas_dev[4], const plk_fr *beta, const plk_fr *gamma,
                                          uint32_t log_n, void *z_values_dev, void *stream) {
    if (!ctx || !wires_dev || !sigmas_dev || !beta || !gamma || !z_values_dev || log_n > MAX_LOG_N) { set_error("plk_permutation_grand_product_dev: bad argument"); return PLK_ERR_ARG; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const uint64_t N = 1ull << log_n;
    DevBuf tmp;
    PLK_TRY(tmp.reserve(2 * N * sizeof(Fr)));
    HFr hb, hg; memcpy(hb.l, beta->l, 32); memcpy(hg.l, gamma->l, 32);
    const PermArgs pa = perm_args(ctx, reinterpret_cast<const Fr *const *>(wires_dev), reinterpret_cast<const Fr *const *>(sigmas_dev), hb, hg, log_n,
                                  tmp.as<Fr>(), tmp.as<Fr>() + N);
    HFr total;
    int32_t rc = grand_product(ctx, pa, (Fr *)z_values_dev, st, "grand product denominator vanished", &total, nullptr);      // round 2's own sequence
    if (hipStreamSynchronize(st) != hipSuccess && rc == PLK_OK) rc = hip_fail(hipGetLastError(), "sync", __FILE__, __LINE__);
    tmp.release();
    return rc;
}

int32_t plk_setup_permutation_dev(plk_ctx *ctx, const void *const vars_dev[4], uint32_t log_n, uint64_t num_vars, void *index_dev, void *const sigmas_dev[4], void *stream) {
    return guarded("plk_setup_permutation_dev", PLK_ERR_HIP, [&]() -> int32_t {
        bool ok = ctx && vars_dev && log_n <= MAX_LOG_N - 2 && num_vars != 0 && (index_dev || sigmas_dev);
        for (int j = 0; ok && j < 4; j++) ok = vars_dev[j] && (!sigmas_dev || sigmas_dev[j]);
        if (!ok) { set_error("plk_setup_permutation_dev: bad argument"); return PLK_ERR_ARG; }
        PLK_HIP(hipSetDevice(ctx->device));
        hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
        const uint64_t N = 1ull << log_n;
        DevBuf idx_buf;                                              // the index is needed either way; the caller's memory where it is asked for
        if (!index_dev) PLK_TRY(idx_buf.reserve((size_t)4 * N * 4));
        const uint32_t *vars[4];
        Fr *sig[4] = {};
        for (int j = 0; j < 4; j++) { vars[j] = (const uint32_t *)vars_dev[j]; if (sigmas_dev) sig[j] = (Fr *)sigmas_dev[j]; }
        int32_t rc = setup_permutation(ctx, vars, log_n, num_vars, index_dev ? (uint32_t *)index_dev : idx_buf.as<uint32_t>(), sigmas_dev ? sig : nullptr, st);
        if (hipStreamSynchronize(st) != hipSuccess && rc == PLK_OK) rc = hip_fail(hipGetLastError(), "sync", __FILE__, __LINE__);
        idx_buf.release();
        return rc; });
}

// the exported entry points: no C++ exception (std::bad_alloc from a host vector of a 2^26 domain) crosses the boundary
int32_t plk_setup_prepare(plk_ctx *ctx, const plk_circuit *c, plk_setup **out) {
    return guarded("plk_setup_prepare", PLK_ERR_HIP, [&] { return setup_prepare_impl(ctx, c, out); });
}
int32_t plk_setup_prepare_host(const plk_circuit *c, plk_setup **out) {
    return guarded("plk_setup_prepare_host", PLK_ERR_FORMAT, [&] { return setup_host_impl(c, out); });
}
int32_t plk_setup_upload(plk_ctx *ctx, plk_setup *s) {
    return guarded("plk_setup_upload", PLK_ERR_HIP, [&] { return setup_upload_impl(ctx, s); });
}
static int32_t not_a_worker(plk_ctx *ctx, const char *who) {
    if (!ctx || !comm_scatter_worker(ctx)) return PLK_OK;
    set_error(std::string(who) + ": this rank serves the owner's commitments (owner-computes mode: call plk_comm_serve; only rank 0 proves)");
    return PLK_ERR_ARG;
}
int32_t plk_setup_write_vk(plk_ctx *ctx, const plk_setup *s, const uint8_t g2_bytes[256], uint8_t *out, uint64_t cap, uint64_t *len) {
    PLK_TRY(not_a_worker(ctx, "plk_setup_write_vk"));
    return guarded("plk_setup_write_vk", PLK_ERR_HIP, [&] { return setup_write_vk_impl(ctx, s, g2_bytes, out, cap, len); });
}
// the `T: Transcript` of prove_by_steps::<_, _, T> (src/plonk.rs:160-169) for every proof of this context; host state only
int32_t plk_ctx_set_transcript(plk_ctx *ctx, const plk_transcript_ops *ops) {
    if (!ctx) { set_error("plk_ctx_set_transcript: null context"); return PLK_ERR_ARG; }
    if (!ops) { ctx->tr_set = false; ctx->tr_ops = plk_transcript_ops{}; return PLK_OK; }
    if (!transcript_ops_complete(ops)) { set_error("plk_ctx_set_transcript: the transcript table has a null callback"); return PLK_ERR_ARG; }
    if (ops->flags & ~(uint32_t)PLK_TRANSCRIPT_CONCURRENT) { set_error("plk_ctx_set_transcript: unknown flag in the transcript table"); return PLK_ERR_ARG; }
    ctx->tr_ops = *ops;
    ctx->tr_set = true;
    return PLK_OK;
}
int32_t plk_prove(plk_ctx *ctx, const plk_setup *S, const plk_circuit *c, uint8_t *proof_out, uint64_t cap, uint64_t *len) {
    PLK_TRY(not_a_worker(ctx, "plk_prove"));
    return guarded("plk_prove", PLK_ERR_HIP, [&]() -> int32_t {
        if (!ctx || !S || !c || !proof_out || !len) { set_error("plk_prove: bad argument"); return PLK_ERR_ARG; }
        WitnessSrc src; src.c = c;
        return prove_impl(ctx, S, src, "plk_prove", proof_out, cap, len); });
}
int32_t plk_prove_witness(plk_ctx *ctx, const plk_setup *S, const plk_fr *witness_host, uint64_t n, uint8_t *proof_out, uint64_t cap, uint64_t *len) {
    PLK_TRY(not_a_worker(ctx, "plk_prove_witness"));
    return guarded("plk_prove_witness", PLK_ERR_HIP, [&] {
        WitnessSrc src; src.host = reinterpret_cast<const HFr *>(witness_host); src.n = n;
        return prove_witness_entry(ctx, S, src, "plk_prove_witness", proof_out, cap, len); });
}
int32_t plk_prove_witness_dev(plk_ctx *ctx, const plk_setup *S, const void *witness_dev, uint64_t n, uint8_t *proof_out, uint64_t cap, uint64_t *len, void *stream) {
    PLK_TRY(not_a_worker(ctx, "plk_prove_witness_dev"));
    return guarded("plk_prove_witness_dev", PLK_ERR_HIP, [&] {
        WitnessSrc src; src.dev = static_cast<const Fr *>(witness_dev); src.n = n; src.caller = (hipStream_t)stream;
        return prove_witness_entry(ctx, S, src, "plk_prove_witness_dev", proof_out, cap, len); });
}
int32_t plk_prove_wtns(plk_ctx *ctx, const plk_setup *S, const uint8_t *wtns, uint64_t wtns_len, uint8_t *proof_out, uint64_t cap, uint64_t *len, uint64_t *bad_out) {
    if (bad_out) *bad_out = ~0ull;
    PLK_TRY(not_a_worker(ctx, "plk_prove_wtns"));
    return guarded("plk_prove_wtns", PLK_ERR_HIP, [&]() -> int32_t {
        if (len) *len = 0;
        if (!ctx || !S || !wtns || !proof_out || !len) { set_error("plk_prove_wtns: bad argument"); return PLK_ERR_ARG; }
        WitnessSrc src;
        size_t payload = 0;
        if (!wtns_container(wtns, wtns_len, &src.n, &payload)) return PLK_ERR_FORMAT;     // plk_wtns_decode's (parse_wtns_bin's) container checks
        src.payload = wtns + payload; src.bad_out_of_file = bad_out;
        return prove_witness_entry(ctx, S, src, "plk_prove_wtns", proof_out, cap, len); });
}
int32_t plk_validate_witness(plk_ctx *ctx, const plk_setup *S, const plk_circuit *c, int32_t *valid, uint64_t *bad_row) {
    return guarded("plk_validate_witness", PLK_ERR_HIP, [&]() -> int32_t {
        if (valid) *valid = 0;
        if (bad_row) *bad_row = ~0ull;
        if (!ctx || !S || !c || !valid) { set_error("plk_validate_witness: bad argument"); return PLK_ERR_ARG; }
        WitnessSrc src; src.c = c;
        return validate_witness_impl(ctx, S, src, "plk_validate_witness", valid, bad_row); });
}
int32_t plk_validate_witness_dev(plk_ctx *ctx, const plk_setup *S, const void *witness_dev, uint64_t n, int32_t *valid, uint64_t *bad_row, void *stream) {
    return guarded("plk_validate_witness_dev", PLK_ERR_HIP, [&]() -> int32_t {
        if (valid) *valid = 0;
        if (bad_row) *bad_row = ~0ull;
        if (!ctx || !S || !witness_dev || !valid) { set_error("plk_validate_witness_dev: bad argument"); return PLK_ERR_ARG; }
        if ((uintptr_t)witness_dev & 15u) { set_error("plk_validate_witness_dev: the witness must be 16-byte aligned"); return PLK_ERR_ARG; }
        WitnessSrc src; src.dev = static_cast<const Fr *>(witness_dev); src.n = n; src.caller = (hipStream_t)stream;
        return validate_witness_impl(ctx, S, src, "plk_validate_witness_dev", valid, bad_row); });
}
int32_t plk_setup_from_polynomials(plk_ctx *ctx, uint64_t n, uint64_t num_inputs, const plk_fr *const selectors[6], const plk_fr *next_step_selector,
                                   const plk_fr *const sigmas[4], uint64_t len, uint32_t flags, plk_setup **out) {
    return guarded("plk_setup_from_polynomials", PLK_ERR_HIP, [&] { return setup_polys_impl(ctx, n, num_inputs, selectors, next_step_selector, sigmas, len, flags, out); });
}
int32_t plk_prove_assembled(plk_ctx *ctx, const plk_setup *s, const plk_fr *const columns[4], uint64_t rows, uint8_t *proof_out, uint64_t cap, uint64_t *len) {
    PLK_TRY(not_a_worker(ctx, "plk_prove_assembled"));
    return guarded("plk_prove_assembled", PLK_ERR_HIP, [&] {
        return prove_assembled_impl(ctx, s, reinterpret_cast<const void *const *>(columns), false, rows, proof_out, cap, len, nullptr); });
}
int32_t plk_prove_assembled_dev(plk_ctx *ctx, const plk_setup *s, const void *const columns_dev[4], uint64_t rows, uint8_t *proof_out, uint64_t cap,
                                uint64_t *len, void *stream) {
    PLK_TRY(not_a_worker(ctx, "plk_prove_assembled_dev"));
    return guarded("plk_prove_assembled_dev", PLK_ERR_HIP, [&] {
        return prove_assembled_impl(ctx, s, columns_dev, true, rows, proof_out, cap, len, (hipStream_t)stream); });
}
int32_t plk_setup_check_permutation(plk_ctx *ctx, const plk_setup *s, plk_copy_report *out) {
    return guarded("plk_setup_check_permutation", PLK_ERR_HIP, [&] { return check_copies_impl(ctx, s, nullptr, false, false, 0, out, nullptr, "plk_setup_check_permutation"); });
}
int32_t plk_check_copies(plk_ctx *ctx, const plk_setup *s, const plk_fr *const columns[4], uint64_t rows, plk_copy_report *out) {
    return guarded("plk_check_copies", PLK_ERR_HIP, [&] {
        return check_copies_impl(ctx, s, reinterpret_cast<const void *const *>(columns), true, false, rows, out, nullptr, "plk_check_copies"); });
}
int32_t plk_check_copies_dev(plk_ctx *ctx, const plk_setup *s, const void *const columns_dev[4], uint64_t rows, plk_copy_report *out, void *stream) {
    return guarded("plk_check_copies_dev", PLK_ERR_HIP, [&] {
        return check_copies_impl(ctx, s, columns_dev, true, true, rows, out, (hipStream_t)stream, "plk_check_copies_dev"); });
}
int32_t plk_comm_serve(plk_ctx *ctx, uint64_t *batches) {
    if (batches) *batches = 0;
    if (!ctx || !comm_scatter_worker(ctx)) { set_error("plk_comm_serve: not a worker rank (rank > 0) of a communicator in scatter mode"); return PLK_ERR_ARG; }
    if (!ctx->srs().pts) { set_error("plk_comm_serve: no key slice resident"); return PLK_ERR_SRS; }
    PLK_TRY(fifo_must_be_empty(ctx, "plk_comm_serve"));
    return guarded("plk_comm_serve", PLK_ERR_HIP, [&] { PLK_HIP(hipSetDevice(ctx->device)); FifoGuard drain(ctx); return serve_impl(ctx, batches); });
}

}  // extern "C"
