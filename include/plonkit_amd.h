/*
 * plonkit_amd — C ABI of the MI355X-native PLONK prover hot path (libplonkit_amd.so).
 *
 * This is the drop-in boundary for the arithmetic that fluidex/plonkit reaches in bellman_ce
 * (reference call sites in parentheses; file:line under /root/reference).  plonkit has no FFI of
 * its own — it links bellman_ce statically — so each entry point below names the Rust call it
 * replaces; INTEGRATION.md shows the `extern "C"` block a plonkit maintainer would add.
 *
 * Conventions
 *   - plk_fr          = 4 x u64 little-endian limbs, MONTGOMERY form (R = 2^256): byte-identical
 *                       to ff_ce's in-memory `Fr`, so a Rust `&[Fr]` can be passed as is.
 *   - plk_g1_affine   = x[4] || y[4], Montgomery Fq; the point at infinity is x = y = 0
 *                       (pairing_ce's G1Affine carries a separate `infinity` flag: repack once).
 *   - plk_g1_jacobian = X || Y || Z, infinity is Z = 0.
 *   - every function returns int32_t: PLK_OK or an error code; text via plk_last_error().
 *     Nothing throws across the boundary.  Calls are blocking unless a stream is passed.
 *   - one plk_ctx drives ONE GPU (one process per GPU; multi-GPU = ranks joined by plk_comm_init: the
 *     96-byte partial sums of every commitment are all-gathered over RCCL and added, inside the library).
 *   - `*_dev` entry points take HIP device pointers (e.g. torch tensors' data_ptr()) and a
 *     hipStream_t passed as void* (NULL = the context's own stream); `host` ones take host memory.
 *     The context's stream is NOT ordered against the caller's streams: data a caller's kernel is still writing (a torch op
 *     on torch's stream, say) must be complete before a `_dev` call that passes NULL reads it — synchronise first, or pass the
 *     producing stream, which the call then runs on (the commitments instead wait for an event recorded on it, see below).
 *   - There is NO CPU fallback: without a gfx950 device plk_create fails with PLK_ERR_HIP.
 */
#ifndef PLONKIT_AMD_H
#define PLONKIT_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct { uint64_t l[4]; } plk_fr;
typedef struct { uint64_t x[4], y[4]; } plk_g1_affine;
typedef struct { uint64_t x[4], y[4], z[4]; } plk_g1_jacobian;
typedef struct plk_ctx plk_ctx;

enum {
    PLK_OK = 0,
    PLK_ERR_ARG = 1,        /* null pointer, bad flag                                         */
    PLK_ERR_SIZE = 2,       /* size not a power of two / log_n > 28 (2-adicity of Fr)         */
    PLK_ERR_SRS = 3,        /* no SRS uploaded or SRS shorter than the request                */
    PLK_ERR_HIP = 4,        /* HIP runtime error, or no gfx950 device                         */
    PLK_ERR_UNSAT = 5,      /* witness does not satisfy the circuit ("must satisfy")          */
    PLK_ERR_FORMAT = 6,     /* malformed r1cs / wtns / key / proof bytes                      */
    PLK_ERR_IO = 7
};

const char *plk_last_error(void);
const char *plk_version(void);
int32_t plk_device_count(void);

/* bellman_ce::worker::Worker::new() (src/plonk.rs:41,47,183): the execution resource handle. */
int32_t plk_create(int32_t device, plk_ctx **out);
void plk_destroy(plk_ctx *ctx);
int32_t plk_synchronize(plk_ctx *ctx);

/* ---- SRS: Crs<Bn256, CrsForMonomialForm> kept resident in HBM (src/plonk.rs:53; src/reader.rs:74-77) */
int32_t plk_srs_upload(plk_ctx *ctx, const plk_g1_affine *bases_host, uint64_t n);
int32_t plk_srs_set_dev(plk_ctx *ctx, const void *bases_dev, uint64_t n);       /* borrowed, not copied */
uint64_t plk_srs_size(const plk_ctx *ctx);
/* Crs::crs_42(size, &Worker) generalised (src/plonk.rs:30-48, `plonkit setup`): fills the resident SRS
 * with tau^(start+i)*G, i < n, computed on the GPU; tau = 42 reproduces the reference's local keys. */
int32_t plk_srs_generate(plk_ctx *ctx, uint64_t n, uint64_t start, uint32_t tau);
int32_t plk_srs_generate_fr(plk_ctx *ctx, uint64_t n, uint64_t start, const plk_fr *tau);     /* any tau (test keys only: tau is public) */
int32_t plk_srs_download(plk_ctx *ctx, uint64_t offset, uint64_t n, plk_g1_affine *out_host);
/* optional: builds now what the first commitment against the resident key(s) would build — the fixed-base table of the
 * MSM (15 shifted copies of the points, ~40 ms at 2^20 points).  A host program calls it on a second thread while it is
 * still parsing the circuit (the `plonkit` binary does); without it the first commitment pays for the table.           */
int32_t plk_srs_precompute(plk_ctx *ctx);
/* SEVERAL PROOFS IN FLIGHT ON ONE GPU.  SetupForProver::prove takes &self (src/plonk.rs:132-176): nothing stops a Rust host from
 * proving from two threads against one setup, and on this hardware it pays — the strict challenge chain of one proof leaves
 * latency-bound stretches (bucket-reduction tails, host round trips, small point-wise launches: ~3.5 ms of a 2^20 proof) that the
 * kernels of a second proof fill.  The unit of concurrency is the context: one plk_ctx per host thread (a context is NOT
 * thread-safe), any number of contexts per device, ONE plk_setup shared by all of them (its lazily cached extensions are
 * filled under a lock), one plk_circuit per witness.  plk_ctx_share_srs makes `dst` borrow `src`'s resident key(s) and MSM
 * fixed-base table(s) instead of building its own (0.94 GiB and ~40 ms per key at 2^20 points): `src` builds what is missing,
 * keeps ownership and refuses to replace a key that a borrower holds (PLK_ERR_ARG; a Lagrange-form key it did not have when the
 * loans were made may still be installed — the borrowers do not see it, share again for that).  Destroying `src` before its
 * borrowers is safe: the key and the tables outlive it until the last borrower returns its loan (plk_destroy / a key of its own).
 * A borrower that is given a key of its own (upload / generate / set_dev) simply stops borrowing.
 * plk_ctx_share_srs MUST NOT RUN CONCURRENTLY WITH ANY CALL ON `src` (nor on `dst`): `src` swaps its monomial / Lagrange key slots for the
 * duration of a Lagrange-form commitment, and a loan taken at that moment would lend the wrong key.  Share first, then start the threads.  */
int32_t plk_ctx_share_srs(plk_ctx *dst, plk_ctx *src);

/* ---- Polynomial::{fft,ifft,coset_fft,icoset_fft} over Fr (bellman_ce::plonk::polynomials; driven
 *      from setup() src/plonk.rs:104 and prove_by_steps src/plonk.rs:152-159).
 *      Natural order in and out.  inverse=0: evaluate on coset*<omega_n>; inverse=1: interpolate
 *      (scaled by 1/n, then by coset^-i).  coset == NULL means 1.                                  */
int32_t plk_ntt(plk_ctx *ctx, plk_fr *data_host, uint32_t log_n, int32_t inverse, const plk_fr *coset);
int32_t plk_ntt_dev(plk_ctx *ctx, void *data_dev, uint32_t log_n, int32_t inverse, const plk_fr *coset, void *stream);
/* Polynomial::coset_lde(4): n coefficients -> 4n evaluations on 7*<omega_4n> */
int32_t plk_lde4(plk_ctx *ctx, const plk_fr *coeffs_host, uint32_t log_n, plk_fr *out_4n_host);
int32_t plk_lde4_dev(plk_ctx *ctx, const void *coeffs_dev, uint32_t log_n, void *out_4n_dev, void *stream);
/* The same 4n evaluations of `count` (<= 16) polynomials in the COSET-MAJOR order the prover's round 3 works in:
 * out[p][k * n + r] = f_p(7 * omega_4n^(4 r + k)), k = 0..3 — four n-point coset transforms per polynomial, all of them in
 * one launch per pass (prove_by_steps' ~18 coset_lde(4) calls, src/plonk.rs:152-159).  A permutation of plk_lde4_dev's output;
 * exposed so that the layout is testable on its own.                                                                      */
int32_t plk_lde4_coset_major_dev(plk_ctx *ctx, const void *const *coeffs_dev, uint32_t count, uint32_t log_n, void *const *out_4n_dev, void *stream);
/* The way back (round 3 of prove_by_steps: Polynomial::icoset_fft at 4n, src/plonk.rs:152-159): 4n values in that coset-major order
 * -> the 4n coefficients in natural order, in place (four inverse n-point coset transforms in one launch per pass + a 4-point combine).
 * Test hook like the function above.                                                                                              */
int32_t plk_icoset4_coset_major_dev(plk_ctx *ctx, void *data_4n_dev, uint32_t log_n, void *stream);

/* ---- kate_commitment::commit_using_monomials -> multiexp::dense_multiexp (src/plonk.rs:122-124 and
 *      the 11 commitments of prove): sum_i scalars[i] * srs[base_offset + i], scalars Montgomery Fr.
 *      One pass of the kernels takes up to 2^24 terms; plk_msm_g1, _dev and _partial_dev (and plk_prove) cut longer
 *      vectors into successive pieces themselves, the _batch_dev and _enqueue_dev entry points return PLK_ERR_SIZE. */
int32_t plk_msm_g1(plk_ctx *ctx, const plk_fr *scalars_host, uint64_t n, uint64_t base_offset, plk_g1_affine *out);
int32_t plk_msm_g1_dev(plk_ctx *ctx, const void *scalars_dev, uint64_t n, uint64_t base_offset, plk_g1_affine *out, void *stream);
/* `count` commitments of equal length against the same bases in one pass of the kernels (the 4 wire /
 * 4 quotient / 2 opening commitments of a proof, the 11 of a verification key)                       */
int32_t plk_msm_g1_batch_dev(plk_ctx *ctx, const void *const *scalars_dev, uint32_t count, uint64_t n, uint64_t base_offset, plk_g1_affine *out, void *stream);
/* the same sum left in Jacobian form, for cross-rank combination (multi-GPU shards) */
int32_t plk_msm_g1_partial_dev(plk_ctx *ctx, const void *scalars_dev, uint64_t n, uint64_t base_offset, plk_g1_jacobian *out, void *stream);
/* enqueue only (no host sync); finish with _finish.  The pair is a FIFO of depth THREE: the context owns three sets of
 * MSM scratch, result buffers and streams, so two more commitments can be enqueued before the first is finished — the
 * accumulation of commitment k then shares the GPU with the latency-bound bucket reduction of k-1 and the digit /
 * partition kernels of k+1 (2^20 terms: 1.39 ms per commitment back to back, 1.46-1.50 with two in flight, 1.66 one
 * at a time).  A slot is taken lowest index first: a caller that keeps two in flight never allocates the third set.
 * `stream` is where the scalars were produced: the kernels run on the slot's own stream after an event recorded there,
 * and the scalars must stay untouched until the matching _finish.  A fourth enqueue, or a finish with nothing in
 * flight, returns PLK_ERR_ARG.                                                                                      */
int32_t plk_msm_g1_enqueue_dev(plk_ctx *ctx, const void *scalars_dev, uint64_t n, uint64_t base_offset, void *stream);
int32_t plk_msm_g1_finish(plk_ctx *ctx, plk_g1_jacobian *out);
/* the same FIFO with a BATCH of `count` (<= 8) commitments of equal length against the same bases per slot — the shape of the
 * prover's rounds (4 wire, 4 quotient, 2 opening commitments): one pass of the kernels serves the whole batch.
 * _finish_batch returns the count Jacobian sums in order; _finish_batch_sharded additionally runs the context's combiner
 * (plk_comm_init / plk_set_commit_shard: one exchange for the batch) and returns affine points.                           */
int32_t plk_msm_g1_enqueue_batch_dev(plk_ctx *ctx, const void *const *scalars_dev, uint32_t count, uint64_t n, uint64_t base_offset, void *stream);
int32_t plk_msm_g1_finish_batch(plk_ctx *ctx, plk_g1_jacobian *out, uint32_t count);
int32_t plk_msm_g1_finish_batch_sharded(plk_ctx *ctx, plk_g1_affine *out, uint32_t count);
/* tracing hook: HIP events around the bucket-accumulation kernel of the last MSM (bench roofline) */
int32_t plk_set_kernel_timing(plk_ctx *ctx, int32_t on);
int32_t plk_msm_last_kernel_ms(plk_ctx *ctx, float *accumulate_ms);
/* DIAGNOSTIC, not part of the computing interface: which dispatch shape the commitment (or batch) finished last on this context
 * took — what tests/test_gpu_msm_shapes.py asserts before it looks at the result, so that a moved threshold fails loudly instead
 * of silently shifting what a test covers.  Plain integers stored in the commitment's slot where the decisions are made (at
 * enqueue; the fallback of a short commitment at its finish): no launch, no synchronisation, no device memory.  The values
 * name internals that may change with any release.  PLK_ERR_ARG before the first finished commitment.                      */
enum { PLK_MSM_PATH_EMPTY = 0,           /* zero terms: nothing was launched                                                   */
       PLK_MSM_PATH_NAIVE = 1,           /* one double-and-add per term (fewer than 4096 terms and the short path not wanted)  */
       PLK_MSM_PATH_SHORT = 2,           /* the short-commitment kernels (all 15 table copies)                                 */
       PLK_MSM_PATH_SHORT_FALLBACK = 3,  /* short, a bucket list overflowed, run again by the kernels the other fields describe */
       PLK_MSM_PATH_ORDINARY = 4 };      /* the bucket pipeline                                                                */
typedef struct plk_msm_shape {
    uint32_t path;                       /* PLK_MSM_PATH_*                                                                     */
    uint32_t batch;                      /* commitments sharing the launches                                                   */
    uint32_t table_copies;               /* shifted copies of the key a commitment addresses: 15, 5, 3 or 1                    */
    /* the bucket pipeline only (0 on the naive and short paths, and for a fallback of fewer than 4096 terms):                 */
    uint32_t window_bits, windows;       /* c and floor(254 / c) + 1                                                           */
    uint32_t bucket_sets;                /* per commitment: windows / table_copies                                             */
    uint32_t fine_bits, coarse_bins;     /* buckets per task = 2^fine_bits; bins per bucket set                                */
    uint32_t accumulate_variant;         /* 0 equal pieces per lane, 2 lanes own buckets (1: a measurement build, retired)    */
    uint32_t prephase;                   /* 1 recoding fused with the partition (digits stay in registers), 2 through the digit array */
    uint32_t reduce_lanes;               /* per task of the bucket reduction: 4 = quads of lanes (one wave per task), 16 or 32 lanes */
    /* the last call of plk_msm_g1 / _dev / _partial_dev, if no other commitment finished since (otherwise 1 and the length):  */
    uint32_t pieces;                     /* passes the call was cut into; the other fields describe the last of them           */
    uint64_t piece_terms;                /* terms per pass (the last one may be shorter)                                       */
} plk_msm_shape;
int32_t plk_msm_last_shape(plk_ctx *ctx, plk_msm_shape *out);
/* DIAGNOSTIC like the above: 1 if the bucket accumulation of the commitment finished last ran the kernel that omits the
 * point-at-infinity test — chosen when the resident key's MSM table holds no such point, which is established each time the
 * table is built (every upload, load, generation or update of a key voids the table) — and 0 otherwise (a key with such a
 * point, a commitment of <= 2^16 terms, the naive and short paths).                                                       */
int32_t plk_msm_last_no_inf(plk_ctx *ctx, uint32_t *out);

/* ---- multiexp::dense_multiexp(&worker, bases, scalars) with the bases as an argument: out = sum_{i<n} scalars[i] * bases[i] for points that
 *      are NOT the resident key.  Every plk_msm_g1* call above sums against the resident key and reads it through the fixed-base table (15
 *      shifted copies of the key: 0.94 GiB and ~40 ms at 2^20 points) — right for a prover that commits to one key thousands of times, wrong
 *      for a one-off sum, and no answer at all for points that must not become the key.  These calls keep no table and need no key:
 *      a front kernel converts the caller's points into a scratch of 64 B per term of the pass (never cached across calls: the caller's
 *      memory may change), and the pass runs the shape of a key without shifted copies — fewer than 4096 terms: one double-and-add per
 *      term; otherwise 13-bit windows below 2^17 terms, 15-bit below 2^19, 17-bit from there, one bucket set per window (plk_msm_last_shape
 *      reports the pass: table_copies = 1).  Costs: DESIGN.md §4.2c.
 *      Bases: the key's in-memory form, 64 bytes x ‖ y Montgomery, (0, 0) = infinity.  Scalars: Montgomery Fr, as for plk_msm_g1_dev.
 *      n = 0 gives infinity and launches nothing.  Synchronous like plk_msm_g1_dev; the work is ordered after `stream` (NULL: the context's).
 *      plk_msm_g1_bases (host pointers: 96 B per term through the context's staging buffer) and _bases_dev cut vectors above 2^24 terms into
 *      passes of 2^24, one at a time, and add the partial sums on the host; _bases_batch_dev (`count` <= 8 scalar vectors against the same
 *      bases, one pass of the kernels, `out` holds count points) returns PLK_ERR_SIZE above 2^24 terms, as plk_msm_g1_batch_dev does.
 *      NO KEY NEEDS TO BE RESIDENT, and nothing about the resident key(s), their table(s), the Lagrange slot or any loan changes: the calls
 *      are allowed on a context whose key is lent or borrowed (plk_ctx_share_srs).  They do not join the FIFO of _enqueue / _finish: a
 *      commitment still in flight on the context is PLK_ERR_ARG.  PLK_ERR_ARG also: null ctx / out, a null pointer with n > 0, a device
 *      pointer that is not 16-byte aligned, unknown flag bits, `count` outside 1..8.
 *      Without PLK_MSM_CHECK_BASES the bases are taken on trust, exactly as plk_srs_upload takes a key: a point off the curve gives some
 *      point, never a fault; *bad_out = UINT64_MAX.  With it every base must be (0, 0) or have x, y < q and y^2 = x^3 + 3 (checked by the
 *      front kernel, before any commitment kernel is launched; a vector of several passes is checked whole first, at the price of converting
 *      it twice): otherwise PLK_ERR_FORMAT with plk_g1_decode_dev's words, *bad_out = the LOWEST refused index, `out` untouched.
 *      The scratch grows only and is freed with the context; a call that had to grow it beyond 2^20 points' worth (64 MiB) frees it before
 *      it returns (1 GiB at 2^24 terms is not left attached to a long-lived context).                                                       */
#define PLK_MSM_CHECK_BASES 1u   /* refuse a base that is neither (0, 0) nor a curve point with coordinates below q */
int32_t plk_msm_g1_bases(plk_ctx *ctx, const plk_g1_affine *bases_host, const plk_fr *scalars_host, uint64_t n,
                         uint32_t flags, plk_g1_affine *out, uint64_t *bad_out /* may be NULL */);
int32_t plk_msm_g1_bases_dev(plk_ctx *ctx, const void *bases_dev, const void *scalars_dev, uint64_t n,
                             uint32_t flags, plk_g1_affine *out, uint64_t *bad_out /* may be NULL */, void *stream);
int32_t plk_msm_g1_bases_batch_dev(plk_ctx *ctx, const void *bases_dev, const void *const *scalars_dev, uint32_t count,
                                   uint64_t n, uint32_t flags, plk_g1_affine *out, uint64_t *bad_out /* may be NULL */, void *stream);

/* ---- Crs::<Lagrange>::from_powers (src/plonk.rs:179-185): inverse NTT over G1 (dump-lagrange)  */
int32_t plk_g1_intt(plk_ctx *ctx, const plk_g1_affine *in_host, uint32_t log_n, plk_g1_affine *out_host);
/* same, from the first 2^log_n points of the resident SRS into a device buffer (64 B per point) */
int32_t plk_g1_intt_srs_dev(plk_ctx *ctx, uint32_t log_n, void *out_dev, void *stream);

/* ---- multi-GPU commitments inside plk_prove / plk_setup_write_vk (the MSM shards, everything else
 *      is replicated).  One process per GPU; rank r keeps only the SRS points [first_index, first_index + plk_srs_size)
 *      resident (plk_srs_upload of its slice, or plk_srs_generate(ctx, n, first_index, tau)), computes every
 *      commitment over that index range and hands the `count` (<= 8) Jacobian partial sums to `combine`, which must
 *      replace them in place by the sums over all ranks — an all_gather of 96 bytes per commitment over RCCL and a
 *      host EC sum (plonkit_amd/sharded.py: ShardedProver); EC addition is not an RCCL reduction op.  All ranks then
 *      hold the same commitments, derive the same challenges and produce the same proof bytes as a single GPU.
 *      combine == NULL switches back to single-GPU commitments.  A Lagrange-form key, if used, is sliced the same way. */
typedef int32_t (*plk_combine_fn)(void *user, plk_g1_jacobian *sums, uint32_t count);
int32_t plk_set_commit_shard(plk_ctx *ctx, uint64_t first_index, plk_combine_fn combine, void *user);

/* ---- the same, with the exchange built in (comm.cpp): the counterpart of `Worker::new()` (src/plonk.rs:41,47,183) for a node
 *      of GPUs is ONE PROCESS PER GPU, each with its own plk_ctx, joined by an RCCL communicator.  A caller in any language
 *      (the Rust host of INTEGRATION.md, the `plonkit` binary of this package) needs no collective library of its own:
 *        rank 0:  plk_comm_unique_id(&id), hand the 128 bytes to the other ranks (file, pipe, env — the caller's choice)
 *        all:     plk_create(device_of_rank) ; plk_comm_init(ctx, rank, world, &id, first_index)
 *                 plk_srs_upload(ctx, key + first_index, n_local)      (or plk_srs_generate(ctx, n_local, first_index, tau))
 *                 plk_setup_prepare / plk_setup_write_vk / plk_prove as on one GPU: identical bytes on every rank
 *      plk_comm_init creates the communicator on the context's device (ncclCommInitRank — collective: every rank must
 *      call it) and installs the built-in combiner: one ncclAllGather of count x 96 bytes on a stream of its own per
 *      batch of commitments, then world-1 host EC additions each (EC addition is not an RCCL reduction op).
 *      RCCL is bound at run time (librccl.so.1); without it these calls return PLK_ERR_HIP and everything else works.
 *      plk_comm_init_tcp is the same combiner over a TCP hub on 127.0.0.1:port (rank 0 listens) for the one case RCCL
 *      refuses — several ranks sharing ONE device, as on a single-GPU test box.                                        */
typedef struct { char bytes[128]; } plk_comm_id;                       /* an ncclUniqueId */
int32_t plk_comm_unique_id(plk_comm_id *out);
int32_t plk_comm_init(plk_ctx *ctx, int32_t rank, int32_t world, const plk_comm_id *id, uint64_t first_index);
int32_t plk_comm_init_tcp(plk_ctx *ctx, int32_t rank, int32_t world, uint16_t port, uint64_t first_index);
int32_t plk_comm_set_shard(plk_ctx *ctx, uint64_t first_index);         /* same communicator, another slice of the key */
/* Two ways to use the ranks of a communicator (bellman's Worker, src/plonk.rs:41,47,183, has one: threads of one address space):
 *   PLK_SHARD_REPLICATE (default)  every rank runs the same plk_prove on the same circuit; only the commitments are split.  The
 *                                  transforms, the quotient and the openings are done G times over (Amdahl: <= 2.5x at 2^20).
 *   PLK_SHARD_SCATTER              OWNER COMPUTES: rank 0 alone runs plk_prove / plk_setup_write_vk.  For every batch of commitments
 *                                  it sends each other rank that rank's slice of the scalar vectors (N/G x 32 B per vector: 4 MiB per
 *                                  xGMI link at 2^20, 64 MiB at 2^24; grouped ncclSend / ncclRecv) and gets 96 bytes back; the other
 *                                  ranks only hold their slice of the key and sit in plk_comm_serve.  Same proof bytes.  Rank r must
 *                                  hold the key points [r * L, (r + 1) * L), L = the owner's key size (plk_comm_init's first_index).
 * Every rank of a communicator must be in the same mode: PLK_SHARD_MODE=scatter in the environment of all of them, or
 * plk_comm_set_mode on all of them right after plk_comm_init.
 * PLK_SHARD_SCATTER IS EXPERIMENTAL BETWEEN GPUS: its RCCL transport (header broadcast + grouped ncclSend / ncclRecv) has run on one GPU only
 * (plk_comm_selftest, plk_comm_scatter_selftest) and over the TCP tier of the tests — no multi-GPU node has run it.  On an RCCL communicator of
 * more than one rank plk_comm_set_mode(SCATTER) therefore runs plk_comm_selftest first (a collective, like the call itself) and refuses the mode
 * if that fails.  If the owner's plk_prove / plk_setup_write_vk returns an error after a batch went out (PLK_ERR_UNSAT, ...), the batch's exchange
 * is still run, so that the workers stay in step and the communicator stays usable.                                                       */
#define PLK_SHARD_REPLICATE 0
#define PLK_SHARD_SCATTER 1
int32_t plk_comm_set_mode(plk_ctx *ctx, int32_t mode);
/* worker ranks (rank > 0) of a scatter-mode communicator: commit whatever the owner sends against this context's key slice until the
 * owner calls plk_comm_stop_workers (returns PLK_OK) or goes away (PLK_ERR_HIP / PLK_ERR_IO).  *batches = batches served.            */
int32_t plk_comm_serve(plk_ctx *ctx, uint64_t *batches);
int32_t plk_comm_stop_workers(plk_ctx *ctx);                            /* owner: ends every worker's plk_comm_serve */
/* every rank: one header broadcast + one grouped ring step (send to rank + 1, receive from rank - 1) over the RCCL communicator, checked
 * byte by byte — the transport of owner-computes mode, exercised before the mode is trusted on a new node (works with one rank too).       */
int32_t plk_comm_selftest(plk_ctx *ctx);
/* one GPU, RCCL communicator of ONE rank, key of >= 2^log_n points: the scatter step of owner-computes mode through the real RCCL branch
 * (comm_send_work / comm_recv_work, rank 0 receiving its own share), `iterations` times, with the scalars STILL BEING WRITTEN on the context's
 * stream when the step is called — the ordering the TCP tier cannot test.  The commitment of what arrived must equal the commitment of the
 * vector itself; *mismatches = iterations where it does not (0 is the pass).  No reference counterpart (bellman's Worker shares memory).    */
int32_t plk_comm_scatter_selftest(plk_ctx *ctx, uint32_t log_n, uint32_t iterations, uint32_t *mismatches);
/* ranks RCCL itself counts in the context's communicator (ncclCommCount); 0 without an RCCL communicator — the multi-GPU bench line prints it */
int32_t plk_comm_nccl_count(const plk_ctx *ctx, int32_t *count);
int32_t plk_comm_destroy(plk_ctx *ctx);                                 /* back to single-GPU commitments */
/* plk_msm_g1_finish + the combiner: the commitment over all ranks' shards (each rank enqueued its own slice), affine */
int32_t plk_msm_g1_finish_sharded(plk_ctx *ctx, plk_g1_affine *out);
/* the combiner on its own (no context, no GPU): the TCP transport opened directly, and the plk_combine_fn it serves —
 * plk_set_commit_shard(ctx, first, plk_comm_combine, comm) is what plk_comm_init_tcp does.  Used by the CPU tests. */
int32_t plk_comm_open_tcp(int32_t rank, int32_t world, uint16_t port, void **comm_out);
int32_t plk_comm_combine(void *comm, plk_g1_jacobian *sums, uint32_t count);
void plk_comm_close(void *comm);
/* test tier: the scatter step of owner-computes mode on HOST buffers over a plk_comm_open_tcp communicator (same header, shares and sequence
 * numbers as the device path).  Rank 0 sends vecs[0..count) (n elements of 32 B; count = 0: the stop message); rank r > 0 blocks for the next
 * message and receives count_out x len_out x 32 bytes, len_out = its share [r * slice, min((r + 1) * slice, n)).                        */
int32_t plk_comm_scatter_host(void *comm, const void *const *vecs, uint32_t count, uint64_t n, uint64_t slice,
                              void *mine, uint64_t mine_cap, uint32_t *count_out, uint64_t *len_out);
int32_t plk_comm_info(const plk_ctx *ctx, int32_t *rank, int32_t *world, uint64_t *exchanges);

/* ---- Lagrange-form key: Crs<E, CrsForLagrangeForm> (L_i(tau)*G, i < N), the optional `-l` key of `plonkit prove`
 *      (src/bin/main.rs:384-391; src/plonk.rs:138-146: with it, prove() commits the witness and grand-product
 *      polynomials from their evaluations — commit_using_values — instead of their coefficients).  A second resident
 *      SRS with its own fixed-base table; while one is set, plk_prove uses it for those 5 commitments and requires
 *      its size to equal the circuit's domain.  The proof bytes are the same either way.
 *      set_dev: points already on the device, e.g. the output of plk_g1_intt_srs_dev (not copied, must stay alive). */
int32_t plk_srs_lagrange_upload(plk_ctx *ctx, const plk_g1_affine *bases, uint64_t n);
int32_t plk_srs_lagrange_set_dev(plk_ctx *ctx, const void *bases_dev, uint64_t n);
int32_t plk_srs_lagrange_clear(plk_ctx *ctx);
uint64_t plk_srs_lagrange_size(const plk_ctx *ctx);

/* ---- host-side G1 helpers (pure CPU, usable without a GPU) ---------------------------------- */
int32_t plk_g1_sum_jacobian(const plk_g1_jacobian *parts, uint64_t n, plk_g1_affine *out);
int32_t plk_g1_on_curve(const plk_g1_affine *p);                       /* 1 / 0                   */
/* big-endian canonical 64-byte encoding of Proof/VerificationKey/Crs::write     */
int32_t plk_g1_to_bytes(const plk_g1_affine *p, uint8_t out[64]);
int32_t plk_g1_from_bytes(const uint8_t in[64], plk_g1_affine *out);
int32_t plk_fr_to_bytes(const plk_fr *a, uint8_t out[32]);
int32_t plk_fr_from_bytes(const uint8_t in[32], plk_fr *out);

/* ---- SRS key files: Crs::read / Crs::write (src/reader.rs:67-89; src/bin/main.rs:341,379), monomial and
 *      Lagrange containers alike.  parse: points == NULL only reports n and the G2 bytes;
 *      every point is range- and curve-checked like Crs::read.  serialize: out == NULL only reports len.  */
int32_t plk_key_parse(const uint8_t *data, uint64_t len, plk_g1_affine *points, uint64_t cap, uint64_t *n_out, uint8_t g2_out[256]);
int32_t plk_key_serialize(const plk_g1_affine *points, uint64_t n, const uint8_t g2[256], uint8_t *out, uint64_t cap, uint64_t *len);
void plk_crs42_g2_bytes(uint8_t out[256]);        /* G2 section of Crs::crs_42: {G2, 42*G2} */

/* ---- SRS key files on the GPU: Crs::read straight into HBM and Crs::write straight out of it (src/reader.rs:67-89;
 *      src/bin/main.rs:341,379).  The 64-byte points are decoded, range- and curve-checked (and encoded) by kernels; the
 *      host only moves file bytes.  A point is refused exactly when plk_key_parse refuses it (pairing_ce's into_affine:
 *      flag bits, x, y < q, y^2 = x^3 + 3; BN254's G1 has cofactor 1, no subgroup check). */
#define PLK_KEY_LAGRANGE 1u   /* the Lagrange-form slot (plk_srs_lagrange_*) instead of the monomial one */
/* Crs::read.  `data`/`len` = the whole key file in host memory (pageable is fine).  Container checks, codes and words exactly as
 * plk_key_parse.  EVERY point of the file is checked, whatever slice is kept.  Kept resident: points [first, first + count)
 * (count = 0: all from `first`) — a rank's slice.  *n_out = points in the file.  A refused point: PLK_ERR_FORMAT with
 * plk_key_parse's words ("read key err: point not on curve"), *bad_out = the LOWEST refused index (UINT64_MAX if none), and the
 * context's resident key(s) and MSM table(s) are exactly what they were before the call.  first > n, first + count > n, an empty
 * slice, unknown flag bits, null ctx / data / n_out: PLK_ERR_ARG.  A context whose key is lent (plk_ctx_share_srs): PLK_ERR_ARG,
 * as plk_srs_upload.  Device memory beyond the kept points: the file goes up in chunks of plk_key_chunk_points() = 2^20 points
 * through two 64 MiB buffers (copy k + 1 beside kernel k) that stay in the context's staging arena — at most 144 MiB with the
 * arena's slack, whatever the size of the key — and the previous key lives until the new one is complete.                     */
int32_t plk_srs_load_key(plk_ctx *ctx, const uint8_t *data, uint64_t len, uint64_t first, uint64_t count, uint32_t flags,
                         uint64_t *n_out, uint8_t g2_out[256], uint64_t *bad_out /* may be NULL */);
/* Crs::write: the resident key (or the Lagrange-form one) as key-file bytes, through the same two buffers; out == NULL only
 * reports len.  No key of that form resident: PLK_ERR_SRS.                                                                      */
int32_t plk_srs_store_key(plk_ctx *ctx, uint32_t flags, const uint8_t g2[256], uint8_t *out, uint64_t cap, uint64_t *len);
/* the two kernels on device pointers (16-byte aligned, else PLK_ERR_ARG), ordered on `stream` like every _dev call.  decode
 * returns its verdict, so it waits for `stream`: PLK_ERR_FORMAT and *bad_out = lowest refused index (points_dev then holds
 * infinity at every refused index), else *bad_out = UINT64_MAX.  One decode at a time per context.                             */
int32_t plk_g1_decode_dev(plk_ctx *ctx, const void *bytes_dev, uint64_t n, void *points_dev, uint64_t *bad_out /* may be NULL */, void *stream);
int32_t plk_g1_encode_dev(plk_ctx *ctx, const void *points_dev, uint64_t n, void *bytes_dev, void *stream);
uint64_t plk_key_chunk_points(void);              /* points per staging chunk of plk_srs_load_key / plk_srs_store_key */
/* Crs::<Lagrange>::from_powers (src/plonk.rs:179-185) without leaving the device: the G1 iNTT of the first 2^log_n resident
 * points becomes the context's Lagrange-form key (`dump-lagrange` = this + plk_srs_store_key(PLK_KEY_LAGRANGE)).               */
int32_t plk_srs_lagrange_from_powers(plk_ctx *ctx, uint32_t log_n);

/* ---- structure checks of the resident key(s).  NO COUNTERPART IN THE REFERENCE: bellman's Crs::read (src/reader.rs:67-89) checks that every
 *      point is on the curve and nothing else, and so does plk_srs_load_key.  A file of curve points that are not P_0, tau P_0, tau^2 P_0, ...
 *      for the tau of its G2 section (truncated and padded, spliced from two ceremonies, paired with the wrong G2 section), or a Lagrange-form
 *      key that belongs to another monomial key, loads without complaint and every proof made from it is silently invalid.  These two calls say so.
 *
 *      plk_srs_check.  P_0 .. P_{n-1} = the resident monomial points (the whole key or a rank's contiguous slice), g2 = {Q_0, Q_1} = the
 *      2 x 128 bytes of the key file's G2 section.  *valid = 1 exactly when
 *        - P_0 is not the point at infinity;
 *        - Q_0 and Q_1 are on the twist, not infinity, and in the subgroup of order r ([r]Q = O, computed on the host inside this call: the
 *          decoding of plk_pairing_check does not check the subgroup and BN254's G2 has a cofactor);
 *        - every link i < n - 1 holds: e(P_{i+1}, Q_0) = e(P_i, Q_1).
 *      The links are established by ONE random linear combination, in the ONE-COMMITMENT FORM: rho = keccak256("plk_srs_check" || seed) mod r
 *      (hashed again while it is zero), the vector rho^i, i < n, is filled on the device, T = sum_i rho^i P_i is one pass of the commitment
 *      pipeline (plk_msm_g1_dev), and on the host A = T - P_0, B = rho (T - rho^(n-1) P_{n-1}); accepted iff e(A, Q_0) e(-B, Q_1) = 1
 *      (sum_{i<n-1} rho^i P_{i+1} = (T - P_0) / rho: one commitment gives both sums).  A broken link makes the error a nonzero polynomial of
 *      degree < n in rho, so a bad key is accepted with probability <= n / r < 2^-225 (n <= 2^28).  n = 1: only the conditions on P_0 and g2.
 *      ON A SLICE THE LINK INTO IT FROM THE PREVIOUS RANK'S LAST POINT IS NOT COVERED (and nothing ties P_0 of a slice to its global index).
 *      seed == NULL: 32 bytes from the OS (getrandom).  The same seed gives the same rho and the same verdict; a caller who fixes the seed
 *      BEFORE the key is chosen keeps the bound, one who publishes it first does not.
 *      *bad_out: UINT64_MAX for a valid key; 0 when P_0 is infinity; with PLK_KEY_LOCATE on a key whose links fail, the lowest i with
 *      P_{i+1} != tau P_i, found by bisection with the same check on sub-ranges (base_offset = lo, the same vector from index 0: at most n further
 *      commitment terms and ~log2 n pairing checks); without the flag, or when g2 itself is refused, UINT64_MAX.
 *      PLK_OK with *valid = 0 / 1 for every well-formed input — a wrong key is a verdict, not an error.  PLK_ERR_ARG: null ctx / g2 / valid,
 *      unknown flag bits, a commitment still in flight on the context, a G2 encoding that is out of range or not on the twist ("G2 point not
 *      on the twist", as plk_pairing_check).  PLK_ERR_SRS: no key resident.  PLK_ERR_SIZE: more than 2^28 points.  PLK_ERR_IO: getrandom failed.
 *      The call only reads the key: allowed on a borrowed key (plk_ctx_share_srs) and on a plk_srs_set_dev key; the resident key(s), the
 *      Lagrange slot and any loan are what they were.  Side effects: the MSM fixed-base table is built as by a first commitment; the vector
 *      lives in the prover's workspace (see "Workspace" below), so plk_prove_trace has nothing to hand out until the next proof.
 *
 *      plk_srs_lagrange_check.  L_0 .. L_{N-1} = the Lagrange-form slot, N a power of two.  *valid = 1 iff sum_i rho^i L_i = sum_j c_j P_j with
 *      c = iNTT_N(rho^0 .. rho^(N-1)) and rho = keccak256("plk_srs_lagrange_check" || seed) mod r: the same vector, one inverse transform
 *      (plk_ntt_dev's), one commitment against each key, two affine points compared on the host.  No pairing: G1 has cofactor 1.  Same bound.
 *      PLK_ERR_SRS: either key missing, or the monomial key shorter than N.  PLK_ERR_ARG: null ctx / valid, a commitment in flight, or the
 *      context holds a slice: its first index as set by plk_set_commit_shard / plk_comm_init / plk_comm_set_shard is nonzero (tying the two
 *      forms needs the whole prefix).  ONLY THAT INDEX IS LOOKED AT: the context does not remember that plk_srs_load_key(first != 0) or
 *      plk_srs_generate(n, start != 0, ..) gave it a slice; such a pair of keys is simply refused (PLK_OK, *valid = 0).
 *      PLK_ERR_SIZE: N not a power of two.
 *      Workspace: the vector (32 B per point) and its 1 MiB table live in the prover's grows-only workspace for the duration of a call.  A call
 *      that had to GROW that workspace frees it again before it returns (the next proof allocates what it needs), so a one-off check of a 2^26-point
 *      key does not leave 2 GiB attached to a long-lived context; a workspace that was already large enough is reused and kept. */
#define PLK_KEY_LOCATE 2u   /* on a refused monomial key, find the lowest broken link */
int32_t plk_srs_check(plk_ctx *ctx, const uint8_t g2[256], const uint8_t seed[32] /* NULL: OS randomness */,
                      uint32_t flags, int32_t *valid, uint64_t *bad_out /* may be NULL */);
int32_t plk_srs_lagrange_check(plk_ctx *ctx, const uint8_t seed[32] /* NULL: OS randomness */, int32_t *valid);
/* plk_srs_check for a CANDIDATE key: n points in device memory (the key's in-memory form, 16-byte aligned) that are NOT installed — to judge a
 * key before it replaces the resident one, on a context whose key is lent, or in the middle of proving.  Same rules, same rho
 * ("plk_srs_check" ‖ seed), same one-commitment form, same flags, codes and verdict convention: for the same points, g2 and seed it returns
 * the *valid and *bad_out of plk_srs_check on those points made resident.  The commitment and the sub-range commitments of the bisection go
 * through plk_msm_g1_bases_dev's path (points_dev + lo), P_0 and P_{n-1} are read from points_dev: no key needs to be resident, nothing
 * resident changes and NO FIXED-BASE TABLE IS BUILT.  Waits for `stream` (NULL: the context's), then runs on the context's stream.
 * PLK_ERR_ARG as plk_srs_check, and for a null or misaligned points_dev; PLK_ERR_SRS: n = 0.  Workspace as plk_srs_check; the converted
 * points follow the scratch rule of plk_msm_g1_bases_dev, once for the whole call.                                                          */
int32_t plk_srs_check_points_dev(plk_ctx *ctx, const void *points_dev, uint64_t n, const uint8_t g2[256], const uint8_t seed[32] /* NULL: OS randomness */,
                                 uint32_t flags, int32_t *valid, uint64_t *bad_out /* may be NULL */, void *stream);

/* ---- contributing a secret to a key, with a receipt anyone can check.  NO COUNTERPART IN THE REFERENCE: `plonkit setup` makes the key of the
 *      public tau = 42 (src/plonk.rs:30-48, "development only"), and a downloaded key is read and trusted (src/reader.rs:67-89).  The step of an
 *      updatable SRS is the third option: take any valid key of some tau, multiply tau by a secret s, throw s away.  The new key is sound for a
 *      user who is sure that the old tau OR their own s is unknown.
 *
 *      plk_srs_update.  The resident monomial points P_0 .. P_{n-1} (global indexes first .. first + n - 1: a rank's slice, as
 *      plk_srs_generate(n, start, ..)) become P'_i = s^(first + i) P_i: one GLV scalar multiplication per point on the device, the scalar formed
 *      in the lane from a two-level table of s that is zeroed before the call returns; infinity stays infinity.  g2_new = {Q_0, s Q_1} and
 *      receipt = S1 || S2 with S1 = s G1 (64 bytes), S2 = s Q_0 (128 bytes), in the key file's encodings, are computed on the host.
 *      s: Montgomery form, 0 < s < r (else PLK_ERR_ARG); NULL: 32 bytes from the OS (getrandom), reduced mod r, drawn again while zero —
 *      that s exists nowhere once the call returns (every host copy is wiped with explicit_bzero).  Ranks that update slices of one key
 *      must use ONE s: rank 0 draws it, or every rank passes the same.
 *      Checked before anything is computed, with nothing changed on refusal: first + n <= 2^28 (the table's reach; PLK_ERR_SIZE, checked
 *      before s and the G2 section are looked at); the G2 section as plk_srs_check checks it (on the twist, not infinity, [r]Q = O; PLK_ERR_ARG); the key is not lent to
 *      another context (plk_ctx_share_srs) and no commitment is in flight (PLK_ERR_ARG).  PLK_ERR_SRS: no key resident.
 *      The result is written to a new buffer that becomes the context's OWN key after the last chunk succeeded — also when the old key was a
 *      borrowed one or the caller's device memory (plk_srs_set_dev), which is never written.  On success the MSM table of the old key is void
 *      and the Lagrange-form slot is cleared (the old Lagrange-form key no longer belongs).  On any failure the key, its table, the Lagrange
 *      slot, any loan, g2_new and receipt are what they were.  Device memory of the call: the new key, an XYZZ scratch of at most 512 MiB, 1 MiB.
 *
 *      plk_srs_update_receipt.  The host half on its own (no device): g2_new and receipt for a given s.  A rank that updates a slice with the
 *      s rank 0 drew uses it.  s == NULL is PLK_ERR_ARG here.
 *
 *      plk_srs_update_verify.  The NEW key resident, whole prefix (first = 0); old_p01 = P_0, P_1 of the old key (P_1 is not read for a
 *      one-point key).  *valid = 1 exactly when, in this order (*reason = the first rule that failed, PLK_UPDATE_*):
 *        - both G2 sections are sound as plk_srs_check wants them                                     PLK_UPDATE_BAD_G2
 *        - Q_0 is unchanged                                                                           PLK_UPDATE_Q0_CHANGED
 *        - P'_0 = P_0, on the curve and not infinity                                                  PLK_UPDATE_P0_CHANGED
 *        - S1 decodes, is on the curve and not infinity                                               PLK_UPDATE_BAD_S1
 *        - S2 decodes, is on the twist, in the subgroup and not infinity                              PLK_UPDATE_BAD_S2
 *        - e(S1, Q_0) = e(P_0, S2): S1 and S2 hold the same s                                         PLK_UPDATE_RECEIPT_SPLIT
 *        - e(P'_1, Q_0) = e(P_1, S2): the G1 side moved by s (skipped for a one-point key)            PLK_UPDATE_P1_MISMATCH
 *        - e(P_0, Q'_1) = e(S1, Q_1): the G2 side moved by s                                          PLK_UPDATE_Q1_MISMATCH
 *        - plk_srs_check(new key, g2_new, seed) accepts (its error bound, its seed convention)        PLK_UPDATE_KEY_STRUCTURE
 *      The products go through the pairing of plk_verify.  WHAT THIS PROVES: the new key is a key of tau' = s tau for the s committed in
 *      S1 / S2, and s != 0 — given that the OLD key was a valid key of tau (check it with plk_srs_check).  WHAT IT DOES NOT: it is no proof
 *      of knowledge of s, and gives nothing against an adaptive last contributor beyond that.  The call only reads (as plk_srs_check).
 *      A G2 section that is out of range or not on the twist is PLK_ERR_ARG with plk_srs_check's words; PLK_ERR_ARG also for null pointers
 *      and a context that holds a slice; PLK_ERR_SRS: no key resident.  Every other wrong input is a verdict (PLK_OK, *valid = 0).
 *
 *      plk_srs_update_check_receipt.  The host half of the verification (no device): every rule but the last, given P'_0 and P'_1.
 *      points = 1 for a one-point key (the [1] entries are not read), else 2.                                                               */
enum {
    PLK_UPDATE_OK = 0,
    PLK_UPDATE_BAD_G2 = 1,
    PLK_UPDATE_Q0_CHANGED = 2,
    PLK_UPDATE_P0_CHANGED = 3,
    PLK_UPDATE_BAD_S1 = 4,
    PLK_UPDATE_BAD_S2 = 5,
    PLK_UPDATE_RECEIPT_SPLIT = 6,
    PLK_UPDATE_P1_MISMATCH = 7,
    PLK_UPDATE_Q1_MISMATCH = 8,
    PLK_UPDATE_KEY_STRUCTURE = 9
};
int32_t plk_srs_update(plk_ctx *ctx, const plk_fr *s /* Montgomery; NULL: 32 bytes from the OS, reduced, redrawn while zero */,
                       uint64_t first, const uint8_t g2_old[256], uint8_t g2_new[256], uint8_t receipt[192]);
/* tracing hook: HIP-event time, milliseconds, of the device work of the last successful plk_srs_update on this context (table of s, the
 * multiplications and the affine pass of every chunk; not the allocations, not the host's G2 arithmetic).  Recorded only while
 * plk_set_kernel_timing is on; PLK_ERR_ARG otherwise.  No counterpart in the reference.                                                  */
int32_t plk_srs_update_last_ms(plk_ctx *ctx, float *out_ms);
int32_t plk_srs_update_receipt(const plk_fr *s, const uint8_t g2_old[256], uint8_t g2_new[256], uint8_t receipt[192]);
int32_t plk_srs_update_verify(plk_ctx *ctx /* NEW key resident, whole prefix, first = 0 */, const plk_g1_affine old_p01[2],
                              const uint8_t g2_old[256], const uint8_t g2_new[256], const uint8_t receipt[192],
                              const uint8_t seed[32] /* NULL: OS randomness */, int32_t *valid, uint32_t *reason /* may be NULL */);
int32_t plk_srs_update_check_receipt(const plk_g1_affine old_p01[2], const plk_g1_affine new_p01[2], uint32_t points,
                                     const uint8_t g2_old[256], const uint8_t g2_new[256], const uint8_t receipt[192],
                                     int32_t *valid, uint32_t *reason /* may be NULL */);

/* ---- RollingKeccakTranscript (src/plonk.rs:10,140,152; spec contrib/template.sol:267-307) ---- */
typedef struct { uint8_t state0[32], state1[32]; uint32_t counter; } plk_transcript;
void plk_transcript_init(plk_transcript *t);
void plk_transcript_absorb_fr(plk_transcript *t, const plk_fr *v);
void plk_transcript_absorb_g1(plk_transcript *t, const plk_g1_affine *p);
void plk_transcript_challenge(plk_transcript *t, plk_fr *out);
void plk_keccak256(const uint8_t *in, uint64_t len, uint8_t out[32]);

/* ---- a transcript of the CALLER's: the `T: Transcript<Fr>` of prove_by_steps::<_, _, T> and verifier::verify::<_, _, T> as a table of
 *      callbacks (src/plonk.rs:160-169 and 198-204: the "rescue" arms, whose RescueTranscriptForRNS lives in franklin-crypto).  THIS LIBRARY
 *      HOLDS NO HASH BUT KECCAK and gains none here: nothing in the rounds depends on which hash the transcript uses, so a host that owns a
 *      correct transcript hands it over and the prover and the host verifier draw their challenges from it.  With no table set everything
 *      runs the built-in RollingKeccakTranscript exactly as before.
 *   The table.    begin = Transcript::new (or new_from_params: `user` carries the parameters) and leaves the new transcript in *state;
 *                 absorb_fr = commit_field_element; absorb_g1 = commit_fe(x), commit_fe(y) — both coordinates in one call, the point at
 *                 infinity arrives as (0, 0); challenge = get_challenge; end releases the state.  Elements cross as everywhere in this ABI:
 *                 ff_ce's in-memory Montgomery Fr, x ‖ y Montgomery Fq — a Rust callback reinterprets them, no conversion.  The table is
 *                 COPIED when it is handed over (`user` and the functions must stay valid, the struct need not).  All five functions are
 *                 required (a null one: PLK_ERR_ARG); unknown flag bits: PLK_ERR_ARG.
 *   Order.        The calls follow prove_by_steps: begin; the public inputs (absorb_fr each); the 4 wire commitments; challenge beta,
 *                 challenge gamma; the grand-product commitment; challenge alpha; the 4 quotient commitments; challenge z; the 11 values
 *                 a b c d at z, d at z omega, sigma_1..3 at z, t(z), r(z), z(z omega); challenge v; — the prover stops here: end.  The
 *                 verifier goes on: W_z, W_z_omega, challenge u, end.  With one public input that is 27 calls for the prover, begin included and
 *                 end not, and 30 for the verifier.
 *   Failure.      A callback returns 0 for success.  Anything else ends the library call with PLK_ERR_IO and words that name the callback
 *                 and its position ("... the transcript's absorb_g1 callback (call 3 after begin) returned -7").  A challenge whose limbs
 *                 are not below r is refused with PLK_ERR_ARG before any arithmetic, on the host or the device, consumes it.  After the
 *                 first failure no callback but end is called.  EVERY SUCCESSFUL begin IS FOLLOWED BY EXACTLY ONE end, on every way out:
 *                 an unsatisfied witness, a HIP error, a refused challenge, a failed callback.  (A begin that fails gets no end.)
 *                 The prover's own refusals of a challenge keep their code and words whatever the transcript: "challenge z = 0",
 *                 "challenge z = 1", "grand product denominator vanished ..." — PLK_ERR_UNSAT, the context stays usable; the verifier's
 *                 z^N = 1 stays a verdict (*valid = 0).
 *   Threads.      The prover and plk_verify_with / plk_verify_terms_with call back on the calling thread, at the points where the host
 *                 already waits for a commitment; launches, streams and the background stream are what they are under Keccak.
 *                 plk_verify_many_with runs begin .. end of DIFFERENT proofs from its up to 16 host threads at once when the table's
 *                 flags hold PLK_TRANSCRIPT_CONCURRENT, and from the calling thread only, one proof after the other, without it.
 *   plk_ctx_set_transcript.  Per context, like the key: every proving entry point of the context (plk_prove, plk_prove_witness, _witness_dev,
 *                 _wtns, plk_prove_assembled, _assembled_dev) then takes its challenges from the table; plk_prove_trace follows the last proof
 *                 as before.  NULL restores Keccak.  Several contexts of one device may hold different tables; in replicate mode each rank's
 *                 context calls its own.  Both key forms (monomial only, and with a Lagrange-form key) give the same bytes under any
 *                 transcript.
 *   plk_verify_with, plk_verify_terms_with.  plk_verify_ex and plk_verify_terms under the caller's transcript (ops == NULL: exactly those
 *                 calls): same parser, same refusals, same words, and a refused key or proof never reaches begin.
 *   plk_verify_many_with.  plk_verify_many with its host front end running the caller's transcript per proof; the kernels are the same.
 *                 verdict[i] is what plk_verify_with says about proof i (PLK_VERDICT_MALFORMED for a proof it refuses as malformed); a
 *                 failed callback or a refused challenge ends the whole call with that proof's error, "proof <i>: ..." for the lowest
 *                 such i, and launches nothing more.
 *   NOT COVERED.  plk_verify_many_packed, plk_verify_many_dev, plk_verify_front_dev and the plk_verify_mixed* family run Keccak inside their
 *                 front kernel and take no table; a foreign transcript on the device is out of scope.  The `plonkit` binary keeps refusing
 *                 `-t rescue` (exit 101): it has no transcript to hand over.                                                              */
#define PLK_TRANSCRIPT_CONCURRENT 1u   /* begin .. end of different proofs may run on several threads at once (plk_verify_many_with) */
typedef struct plk_transcript_ops {
    void    *user;
    int32_t (*begin)(void *user, void **state);
    int32_t (*absorb_fr)(void *state, const plk_fr *v);
    int32_t (*absorb_g1)(void *state, const plk_g1_affine *p);
    int32_t (*challenge)(void *state, plk_fr *out);
    void    (*end)(void *user, void *state);
    uint32_t flags;
} plk_transcript_ops;
int32_t plk_ctx_set_transcript(plk_ctx *ctx, const plk_transcript_ops *ops /* NULL: the built-in Keccak transcript */);
int32_t plk_verify_with(const uint8_t *vk, uint64_t vk_len, const uint8_t *proof, uint64_t proof_len, uint32_t flags,
                        const plk_transcript_ops *ops, int32_t *valid);
int32_t plk_verify_terms_with(const uint8_t *vk, uint64_t vk_len, const uint8_t *proof, uint64_t proof_len, uint32_t flags,
                              const plk_transcript_ops *ops, plk_g1_affine points[25], plk_fr scalars[25], int32_t *early);

/* ---- verifier (pure CPU, as in the reference): verifier::verify::<E,P,RollingKeccakTranscript>(&proof,&vk,None)
 *      behind plonk::verify (src/plonk.rs:189-210; CLI src/bin/main.rs:425-437).  Takes the bytes of vk.bin and
 *      proof.bin; *valid = 1/0.  Malformed files (short, point off the curve, scalar >= r)
 *      return PLK_ERR_ARG — the reference panics in its readers at that point.  The final check
 *      e(A, g2[0]) * e(B, g2[1]) == 1 is a real BN254 optimal-ate pairing (pairing.cpp), no trapdoor.          */
int32_t plk_verify(const uint8_t *vk, uint64_t vk_len, const uint8_t *proof, uint64_t proof_len, int32_t *valid);
/* plonk::verify with options.  PLK_VERIFY_STRICT_INPUTS: refuse keys with num_inputs = 0, as the Solidity verifier the reference
 * generates does (contrib/template.sol:697 `require(vk.num_inputs >= 1)`).  bellman's Rust verifier behind `plonkit verify`
 * (src/plonk.rs:189-210) has no such requirement as far as this package can tell (UNPINNED: the reference holds no zero-input
 * fixture), so plk_verify accepts them by default; it applies the strict rule when the environment variable
 * PLK_VERIFY_STRICT_INPUTS is set (to anything but 0).  Unknown flag bits: PLK_ERR_ARG.                                          */
#define PLK_VERIFY_STRICT_INPUTS 1u
int32_t plk_verify_ex(const uint8_t *vk, uint64_t vk_len, const uint8_t *proof, uint64_t proof_len, uint32_t flags, int32_t *valid);
/* e(a, g2_a) * e(b, g2_b) == 1 ?   G2 as 128 bytes x.c1|x.c0|y.c1|y.c0 big-endian (the key/vk file encoding) */
int32_t plk_pairing_check(const plk_g1_affine *a, const uint8_t *g2_a, const plk_g1_affine *b, const uint8_t *g2_b, int32_t *is_one);

/* ---- many proofs of one verification key, on the GPU (verify_many.hip).  NO COUNTERPART IN THE REFERENCE: plonk::verify (src/plonk.rs:189-210)
 *      takes one proof on one host thread, and so does plk_verify.  These calls verify EACH proof exactly and on its own: verdict i is what
 *      plk_verify_ex says about proof i.  No random linear combination across proofs, no shared pairing, no probabilistic bound; a bad proof
 *      in a batch is named directly.
 *
 *   plk_vk_load.   Parses vk.bin exactly as plk_verify_ex does (src/plonk.rs:189-210: same refusals, same words, PLK_ERR_ARG); flags takes
 *                PLK_VERIFY_STRICT_INPUTS, unknown bits are PLK_ERR_ARG.  Builds ON THE HOST, with the steps of pairing.cpp's Miller loop, the
 *                line table of g2[0] and g2[1] — slope and intercept of every doubling / addition step, 64 + popcount(6u + 2 - 2^64) + 2 lines
 *                per point — and uploads it with the key's 11 commitments and the generator.  The lines do not depend on the G1 argument, so
 *                the device never does twist arithmetic or an Fq2 inversion, and every exceptional case of a strange G2 point (infinity, not
 *                in the subgroup) is decided by the host code plk_verify runs.  Read-only after load: usable from several contexts of the
 *                device it was loaded on (another device: PLK_ERR_ARG), like plk_setup.  No counterpart in the reference.
 *   plk_verify_many.  Blocks.  verdict[i] = 1 / 0 exactly when plk_verify_ex(vk, proof_i, flags) returns PLK_OK with *valid = 1 / 0;
 *                verdict[i] = PLK_VERDICT_MALFORMED exactly when it returns PLK_ERR_ARG for that proof — a malformed proof is a verdict and
 *                does not end the batch.  *first_bad = the lowest i with verdict[i] != 1, else UINT64_MAX.  count == 0: PLK_OK, nothing is
 *                launched.  Null ctx / vk / verdict / first_bad / proofs / lens / proofs[i]: PLK_ERR_ARG; a commitment in flight on the context:
 *                PLK_ERR_ARG, as the other blocking calls.  Per proof the host (up to 16 threads) runs plk_verify_terms's code; only the proofs
 *                it does not settle go to the device: 25 scalar multiplications, two sums, one pairing product check each.  Device memory is
 *                the context's staging arena: it grows only, and nothing is allocated per call once it has grown (5.5 KB per proof, at most
 *                2^16 proofs per pass).  No counterpart in the reference.
 *                BREAK-EVEN (one MI355X, profiles/verify_many_ab.txt): a call costs ~90 ms whatever the batch up to a few thousand proofs (one
 *                pairing lane per proof), a plk_verify 13 ms.  Measured at 1 / 16 / 256 / 4096 proofs: 90 / 92 / 91 / 120 ms against 13 / 14 /
 *                227 / 3525 ms for a loop of plk_verify on 16 host threads — 256 is the first measured size at which this call wins (the
 *                figures cross near 100).  Below that, prefer plk_verify on host threads.
 *   plk_verify_many_last_ms.  With plk_set_kernel_timing on: [0] host flattening (wall clock of the host threads), then HIP-event times of
 *                [1] upload, [2] scalar multiplications, [3] sums and XYZZ -> affine, [4] pairing checks, [5] download.  Diagnostic.
 *                After plk_verify_many_packed slot [0] is the HIP-event time of the front kernel instead; the other slots keep their meaning.
 *                plk_verify_many_dev does not wait and records no times: after it there is no timed call on the context (PLK_ERR_ARG here).
 *   plk_verify_many_packed.  plk_verify_many from raw bytes, with the front end ON THE DEVICE: count proof.bin images back to back in host
 *                memory, proof i = blob[off[i], off[i + 1]), off has count + 1 entries.  Blocks.  verdict[i] and *first_bad exactly as
 *                plk_verify_many (and so as plk_verify_ex).  One lane per proof parses the bytes (the rules of plk_verify_ex's parser, 11 curve
 *                checks), runs the Keccak transcript, checks the equation at z and writes the 25 scalars of plk_verify_terms; a lane never
 *                reads outside its proof, whatever the counts inside it say, and proofs may start at any byte address.  Every proof of a pass
 *                then goes through plk_verify_many's kernels — one the front end settled as 25 zero terms — and its verdict byte is written
 *                from its state, so nothing returns to the host between the bytes and the verdicts.  Offsets that decrease or reach past
 *                blob_len: PLK_ERR_ARG before anything is launched.  The other refusals, count == 0 and the arena as plk_verify_many; the arena
 *                now also holds the raw bytes of a pass (about 6.7 KB per proof of 1.1 KB).  No counterpart in the reference.
 *                BREAK-EVEN against plk_verify_many (one MI355X, profiles/verify_front_ab.txt): the front kernel is 1.6 - 1.9 ms for any batch up
 *                to 2^16 proofs, the host front end 2 / 27 / 423 ms at 256 / 4096 / 65536.  Measured calls at those sizes: 90.5 / 91.8 / 149.6 ms
 *                against plk_verify_many's 90.9 / 118.3 / 587.6 ms — equal at 256 (the difference is inside the spread), 4096 is the first
 *                measured size at which this call wins by more than plk_verify_many's own spread, 3.9x at 65536.
 *   plk_verify_many_dev.  The same with blob, offsets (8-byte aligned) and verdict bytes in DEVICE memory, ordered on `stream` like every
 *                _dev call: it does not wait for the GPU, and no byte of it passes through the host.  An offset pair that decreases or reaches
 *                past blob_len gives THAT proof PLK_VERDICT_MALFORMED, nothing of it is read, and its neighbours are unaffected.  Null
 *                arguments, a key of another device, a commitment in flight: PLK_ERR_ARG; count == 0 launches nothing.
 *                MEMORY AND ORDER.  Being the one call here that returns before its kernels end, it keeps out of the context's staging arena
 *                (whose users each rely on the earlier ones having waited): its 5.5 KB per proof are a buffer of its own that grows only, and
 *                its kernels run on the context's stream, after what `stream` holds at the call and before what `stream` is given next.  Any
 *                other call on the context may follow without a wait; a second plk_verify_many_dev queues behind the first.  blob, offsets
 *                and verdict must stay allocated until `stream` has passed the call.  No counterpart in the reference.
 *   plk_verify_front_dev.  The front kernel on its own, as plk_pairing_check_many_dev is the pairing kernel on its own: per proof 25
 *                plk_g1_affine and 25 plk_fr, both 16-byte aligned, and a state byte — 1: goes on to the group arithmetic, and points / scalars
 *                equal plk_verify_terms's bit for bit; 0: settled invalid (plk_verify_terms's *early = 0); 2: malformed; for 0 and 2 points
 *                and scalars are zero.  Ordered on `stream`.  No counterpart in the reference.
 *   plk_pairing_check_many_dev.  The pairing kernel on its own: n independent checks e(A_i, Q_0) e(B_i, Q_1) == 1 on device arrays of
 *                plk_g1_affine, one byte of verdict each (1 / 0), ordered on `stream` like every _dev call; pointers 16-byte aligned, else
 *                PLK_ERR_ARG.  g2 = Q_0 | Q_1 decoded and checked as plk_pairing_check does, with the same words.  A G1 entry with x = y = 0 is
 *                infinity (its Miller loop is 1, as on the host); a G1 entry off the curve gets verdict PLK_VERDICT_MALFORMED and the call
 *                still returns PLK_OK.  The first call with a G2 pair the context did not see last builds that pair's table on the host and
 *                waits for `stream` once.  No counterpart in the reference.
 *   plk_verify_terms.  Pure CPU, no context; diagnostic like plk_msm_last_shape.  The flattened form of the two G1 arguments of the final
 *                pairing check of plonk::verify (src/plonk.rs:189-210), one scalar (Montgomery) per distinct point:
 *                  pg = sum_{k < 23} scalars[k] points[k]: the key's 11 commitments (selectors 0..5, next-step 6, permutations 7..10), the
 *                       proof's 11 (wires 11..14, grand product 15, quotient 16..19, W_z 20, W_zw 21), the generator 22;
 *                  px = scalars[23] points[23] + scalars[24] points[24] = -W_z - u W_zw;     accept iff e(pg, g2[0]) e(px, g2[1]) == 1.
 *                *early = 0: the verdict is already "invalid" without any group arithmetic (size or input-count mismatch, z^N == 1, the
 *                equation at z fails, the strict-inputs rule) and points / scalars are zero; *early = 1 otherwise.  Malformed key or proof:
 *                PLK_ERR_ARG with plk_verify_ex's words.                                                                                    */
#define PLK_VERDICT_MALFORMED 2
typedef struct plk_vk plk_vk;
int32_t plk_vk_load(plk_ctx *ctx, const uint8_t *vk, uint64_t vk_len, uint32_t flags, plk_vk **out);
void plk_vk_free(plk_vk *vk);
int32_t plk_verify_many(plk_ctx *ctx, const plk_vk *vk, const uint8_t *const *proofs, const uint64_t *lens, uint64_t count, uint8_t *verdict, uint64_t *first_bad);
/* plk_verify_many under the caller's transcript (see "a transcript of the CALLER's" above; ops == NULL: exactly plk_verify_many).  The packed,
 * _dev, front and mixed calls below run Keccak in their front kernel and take no table.                                                 */
int32_t plk_verify_many_with(plk_ctx *ctx, const plk_vk *vk, const uint8_t *const *proofs, const uint64_t *lens, uint64_t count,
                             const plk_transcript_ops *ops, uint8_t *verdict, uint64_t *first_bad);
int32_t plk_verify_many_last_ms(plk_ctx *ctx, float out_ms[6]);
int32_t plk_pairing_check_many_dev(plk_ctx *ctx, const void *a_dev, const void *b_dev, uint64_t n, const uint8_t g2[256], void *verdict_dev, void *stream);
int32_t plk_verify_terms(const uint8_t *vk, uint64_t vk_len, const uint8_t *proof, uint64_t proof_len, uint32_t flags,
                         plk_g1_affine points[25], plk_fr scalars[25], int32_t *early);
int32_t plk_verify_many_packed(plk_ctx *ctx, const plk_vk *vk, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, uint64_t count, uint8_t *verdict, uint64_t *first_bad);
int32_t plk_verify_many_dev(plk_ctx *ctx, const plk_vk *vk, const void *blob_dev, uint64_t blob_len, const void *off_dev, uint64_t count, void *verdict_dev, void *stream);
int32_t plk_verify_front_dev(plk_ctx *ctx, const plk_vk *vk, const void *blob_dev, uint64_t blob_len, const void *off_dev, uint64_t count, void *points_dev, void *scalars_dev,
                             void *state_dev, void *stream);

/* ---- a mixed batch: proofs of several verification keys in one pass, on the GPU (verify_many.hip).  NO COUNTERPART IN THE REFERENCE: plonk::verify
 *      (src/plonk.rs:189-210) takes one key and one proof.  A verifying service sees one key per circuit, usually all made from one universal
 *      key; a plk_verify_many call per key pays the ~90 ms floor of a call (one lane's pairing chain) once per key while most of the chip
 *      idles.  These calls take the key PER PROOF and keep the exactness contract of the calls above: verdict i is what plk_verify_ex says about
 *      proof i under key key_of[i], with that key's flags.  No random linear combination across proofs, no shared pairing, no regrouping by
 *      key; lanes of one wave may hold different keys and the order of key_of does not matter.
 *
 *   plk_vkset_create.  Key k of the set is keys[k] (1 .. PLK_VKSET_MAX_KEYS keys of the context's device).  n_keys == 0 or above the maximum,
 *                a null pointer, a key of another device: PLK_ERR_ARG.  Each key keeps the flags it was loaded with.  The set owns ONE device
 *                allocation — per key the 160 bytes the front kernel needs, its 12 fixed G1 points and the index of its line table; then the
 *                DISTINCT line tables at one stride (two keys share a table exactly when their 256 G2 bytes are equal; the tables are rebuilt
 *                as plk_vk_load builds them) — and copies of the parsed keys, so the plk_vk objects may be freed afterwards.  Read-only after
 *                creation: usable from several contexts of its device, like plk_vk.  No counterpart in the reference.
 *   plk_vkset_keys, plk_vkset_tables.  The number of keys, and of distinct G2 pairs among them (diagnostic, like plk_msm_last_shape: 1 is
 *                the common case, keys of one universal key).  0 for a null set.
 *   plk_verify_mixed.  plk_verify_many with proof i checked under key key_of[i]: the host front end on up to 16 threads, the survivors packed
 *                WITH their key indices, then vm_mul_mixed_kernel (terms 0..10 and 22 from the lane's key), plk_verify_many's sum and
 *                normalisation kernels unchanged, and the pairing: with one table in the set plk_verify_many's own kernel on that table
 *                (wave-uniform line loads); with several, vm_pairing_mixed_kernel, where every lane walks the table of its key.  Blocks.
 *                verdict[i] and *first_bad as plk_verify_many.  A key_of[i] >= the set's key count: PLK_ERR_ARG before anything is launched.
 *                Null arguments, count == 0, a commitment in flight, passes of 2^16 proofs and the staging arena as plk_verify_many (the arena
 *                holds 4 more bytes per proof).  plk_verify_many_last_ms keeps its slots.  No counterpart in the reference.
 *   plk_verify_mixed_packed.  plk_verify_many_packed likewise: the front end on the device (vm_front_mixed_kernel: the lane's FrontVk through
 *                its key index), the offset-table rules of plk_verify_many_packed, and the key-index rule of plk_verify_mixed.  Blocks.
 *                MEASURED (one MI355X, profiles/verify_mixed_ab.txt): one call over four keys of one G2 pair, interleaved, against four
 *                plk_verify_many_packed calls, at 4 x 64 / 4 x 1024 / 4 x 16384 proofs: 91.0 / 92.9 / 151.7 ms against 362.5 / 365.2 / 393.1 ms.
 *                With four G2 pairs (vm_pairing_mixed_kernel, per-lane line loads): 91.3 / 92.9 / 152.0 ms — no measurable cost.
 *                No counterpart in the reference.
 *   plk_verify_mixed_dev.  plk_verify_many_dev likewise: blob, offsets (8-byte aligned), key indices (uint32_t, 4-byte aligned) and verdict
 *                bytes in DEVICE memory, ordered on `stream`, nothing waits.  The call cannot look at the indices: a proof whose key index is
 *                out of range gets PLK_VERDICT_MALFORMED, nothing of it (not even its offset pair) is read, and its neighbours are unaffected —
 *                the rule of a bad offset pair, which holds here too.  Memory and order as plk_verify_many_dev: the same buffer of its own, the
 *                context's stream between two events; a second call queues behind the first, and behind a plk_verify_many_dev.
 *                No counterpart in the reference.                                                                                            */
typedef struct plk_vkset plk_vkset;
#define PLK_VKSET_MAX_KEYS 1024u
int32_t plk_vkset_create(plk_ctx *ctx, const plk_vk *const *keys, uint32_t n_keys, plk_vkset **out);
void plk_vkset_free(plk_vkset *set);
uint32_t plk_vkset_keys(const plk_vkset *set);
uint32_t plk_vkset_tables(const plk_vkset *set);
int32_t plk_verify_mixed(plk_ctx *ctx, const plk_vkset *set, const uint8_t *const *proofs, const uint64_t *lens, const uint32_t *key_of, uint64_t count, uint8_t *verdict,
                         uint64_t *first_bad);
int32_t plk_verify_mixed_packed(plk_ctx *ctx, const plk_vkset *set, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, const uint32_t *key_of, uint64_t count,
                                uint8_t *verdict, uint64_t *first_bad);
int32_t plk_verify_mixed_dev(plk_ctx *ctx, const plk_vkset *set, const void *blob_dev, uint64_t blob_len, const void *off_dev, const void *key_of_dev, uint64_t count,
                             void *verdict_dev, void *stream);

/* ---- circuit pipeline: circom loaders + transpile + setup + prove ----------------------------
 * plk_circuit mirrors CircomCircuit{r1cs, witness, wire_mapping: None, aux_offset: 1}
 * (src/circom_circuit.rs:41-47).  Loaders follow src/reader.rs:178-241, src/r1cs_file.rs:100-154
 * (r1cs), src/reader.rs:92-175 (witness).  `is_json` selects the parser as the reference does by
 * file suffix (src/reader.rs:93,179).                                                          */
typedef struct plk_circuit plk_circuit;
int32_t plk_circuit_load(const uint8_t *r1cs, uint64_t r1cs_len, int32_t r1cs_is_json,
                         const uint8_t *witness, uint64_t witness_len, int32_t witness_is_json,
                         plk_circuit **out);                            /* witness may be NULL    */
/* synthetic chain circuit of exactly `target_gates` PLONK gates + 1 public input, with witness
 * (xoshiro256** seed, pinned constraint shapes); bench / test input.    */
int32_t plk_circuit_synthetic(uint64_t target_gates, uint64_t seed, plk_circuit **out);
/* the same generator with two more knobs (bench / test input).  witness_seed != 0: the SAME R1CS (it depends on `seed` only) with
 * another satisfying witness — what a prover serving many requests for one circuit sees (CircomCircuit{r1cs, witness},
 * src/circom_circuit.rs:41-47: one r1cs, a witness per proof).  lc_terms = 5..64: "dense" body — every constraint's A side is a
 * linear combination of lc_terms earlier wires plus a constant, the shape of a circom Poseidon round, which the transpiler folds
 * through the d column with q_d_next = -1 (src/circom_circuit.rs:114-131): d, q_d_next and the fourth quotient chunk are live, so a
 * proof does all 11 commitments (the pinned-subset circuit leaves two of them empty).  That chaining rule is unpinned (SURVEY.md
 * A.3).  lc_terms = 0: exactly plk_circuit_synthetic.                                                                            */
int32_t plk_circuit_synthetic_ex(uint64_t target_gates, uint64_t seed, uint64_t witness_seed, uint32_t lc_terms, plk_circuit **out);
/* what = 0: iden3 .r1cs v1 bytes, 1: .wtns v2 bytes (the reference's own input formats,
 * src/r1cs_file.rs:100-154, src/reader.rs:124-175); out == NULL only reports the length.            */
int32_t plk_circuit_export(const plk_circuit *c, int32_t what, uint8_t *out, uint64_t cap, uint64_t *len);
void plk_circuit_free(plk_circuit *c);
/* plonk::analyse (src/plonk.rs:72-93): JSON as serde_json::to_string prints it (src/tests.rs:14) */
int32_t plk_circuit_analyse(const plk_circuit *c, char *out_json, uint64_t cap);

/* SetupForProver (src/plonk.rs:50-55): setup polynomials resident on the GPU */
typedef struct plk_setup plk_setup;
/* SetupForProver::prepare_setup_for_prover (src/plonk.rs:97-119): transpile + setup() = 11 iNTT(N) */
int32_t plk_setup_prepare(plk_ctx *ctx, const plk_circuit *c, plk_setup **out);
/* the same in two calls: the host phase (transpile + columns, pure CPU, no context) may run while another thread is still
 * bringing the GPU up (plk_create, key upload, plk_srs_precompute); plk_setup_upload then moves it to the device
 * (11 uploads, 11 iNTT, the permutation).  plk_setup_prepare == plk_setup_prepare_host + plk_setup_upload.              */
int32_t plk_setup_prepare_host(const plk_circuit *c, plk_setup **out);
int32_t plk_setup_upload(plk_ctx *ctx, plk_setup *s);
void plk_setup_free(plk_setup *s);
uint64_t plk_setup_domain_size(const plk_setup *s);                    /* N = n + 1              */
/* the same N straight from the circuit: transpile only (pure CPU), no columns, no device work — all that `dump-lagrange` needs of
 * prepare_setup_for_prover (src/bin/main.rs:360-381 builds the whole setup to read setup.n) */
int32_t plk_circuit_domain_size(const plk_circuit *c, uint64_t *n_out);
/* make_verification_key + VerificationKey::write (src/plonk.rs:122-124; src/bin/main.rs:501-502).
 * g2_bytes = the 2 x 128 bytes of the key file's G2 section, copied through.                    */
int32_t plk_setup_write_vk(plk_ctx *ctx, const plk_setup *s, const uint8_t g2_bytes[256], uint8_t *out, uint64_t cap, uint64_t *len);
/* SetupForProver::prove(circuit, "keccak") with the monomial key (src/plonk.rs:132-159) followed by
 * Proof::write (src/bin/main.rs:407-408).  Fails with PLK_ERR_UNSAT like the reference's
 * `expect("must satisfy")` (src/plonk.rs:137).                                                  */
int32_t plk_prove(plk_ctx *ctx, const plk_setup *s, const plk_circuit *c, uint8_t *proof_out, uint64_t cap, uint64_t *len);
/* per-phase wall-clock of the last plk_prove on this ctx, milliseconds (tracing hook) */
int32_t plk_prove_timings(const plk_ctx *ctx, double *out_ms, uint32_t cap, uint32_t *count);
/* the vectors between the rounds of the last plk_prove on this ctx (tracing hook: a proof that differs from the reference's
 * is localised to a round).  which: 0..3 wire polynomials a, b, c, d (N coefficients), 4 grand product z (N), 5 quotient t
 * (4N coefficients), 6 linearisation r (N), 7 / 8 the opening quotients behind W_z / W_z_omega (N).  out_host == NULL only
 * reports the length.                                                                                                    */
int32_t plk_prove_trace(plk_ctx *ctx, uint32_t which, plk_fr *out_host, uint64_t cap, uint64_t *n);

/* ---- SetupForProver::validate_witness (src/plonk.rs:127-129) and the R1CS of CircomCircuit::synthesize itself (src/circom_circuit.rs:74-133) */
/* "quickly validate whether a witness is satisfied" (src/plonk.rs:127-129), two ways.
 *
 * plk_validate_witness is the reference's call: the gate-level check of plk_prove on its own.  The witness front end of plk_prove
 * (upload, the transpiler's temporaries on the host or the device) and the gate equation of every row, no key needed, nothing
 * committed.  *valid = 1 / 0; *bad_row = the lowest failing row of the setup's gate table (rows 0 .. num_inputs - 1 are the
 * public-input rows, the gates of constraint 0 follow), UINT64_MAX for a satisfying witness.  A setup from
 * plk_setup_from_polynomials, a circuit without a witness, a circuit that does not match the setup, a setup that is not on the
 * device, a commitment in flight: plk_prove's codes and words.  An unsatisfying witness is a verdict (PLK_OK), not an error.
 *
 * plk_r1cs is the R1CS on the device, and plk_r1cs_check_witness* ask the question on the constraints circom wrote:
 * <A_i, w> * <B_i, w> = <C_i, w> for every i, exactly, mod r.  NO COUNTERPART IN THE REFERENCE (bellman only ever checks its own
 * gates): neither a setup nor a key nor this library's transpiler is involved, so a proving service can screen queued witnesses
 * with it, a circuit author learns WHICH constraint of the .r1cs broke, and its agreement with plk_validate_witness is a test of
 * the transpiler.
 *   plk_r1cs_upload   builds the device layout once per circuit (8-byte terms {wire, coefficient index}, the table of distinct
 *                     coefficients, the lists of short and long linear combinations) and copies it to HBM; the circuit's witness
 *                     is not needed and the circuit may be freed afterwards.  A term on a wire >= num_variables: PLK_ERR_FORMAT.
 *                     Read-only after upload: one plk_r1cs may be used from several contexts of the same device, like a plk_setup.
 *   Witness.          n >= num_variables elements, plk_fr in Montgomery form; extra ones are ignored, fewer is PLK_ERR_ARG.  On the host or
 *                     (_dev) on the device, ordered after the work already enqueued on `stream` (NULL: the context's stream).
 *                     WIRE 0 IS THE CONSTANT 1 WHATEVER witness[0] HOLDS (src/circom_circuit.rs:78,107-113: Index::Input(0) =
 *                     CS::one(), w[0] is never read).  An element that some term reads and that is not a canonical residue:
 *                     PLK_ERR_ARG, "... wire <lowest such wire> holds an element that is not a canonical residue (limbs >= r)";
 *                     elements no term reads are not looked at.
 *   Verdict.          The calls block.  *valid = 1 / 0, *bad_out = the lowest failing constraint or UINT64_MAX.  A constraint with an
 *                     empty A or B and an empty C holds by arithmetic (the reference skips it, :122-123).  A wrong witness is a verdict
 *                     (PLK_OK), not an error, as with plk_srs_check.  A commitment in flight on the context: PLK_ERR_ARG.
 *   Memory.           The 3m values of the linear combinations and the two verdict words live in the context's staging arena (grows
 *                     only), the host witness of plk_r1cs_check_witness beside them; nothing is allocated per call once it has grown.
 *   plk_r1cs_long_lc_terms: linear combinations of at least this many terms are summed by a whole wave, shorter ones by one lane
 *                     (diagnostic, for the tests: it names an internal that may change with any release).                        */
typedef struct plk_r1cs plk_r1cs;
int32_t plk_r1cs_upload(plk_ctx *ctx, const plk_circuit *c, plk_r1cs **out);
void plk_r1cs_free(plk_r1cs *r);
uint64_t plk_r1cs_num_constraints(const plk_r1cs *r);
uint64_t plk_r1cs_num_variables(const plk_r1cs *r);
uint32_t plk_r1cs_long_lc_terms(void);
int32_t plk_r1cs_check_witness(plk_ctx *ctx, const plk_r1cs *r, const plk_fr *witness_host, uint64_t n,
                               int32_t *valid, uint64_t *bad_out /* may be NULL */);
int32_t plk_r1cs_check_witness_dev(plk_ctx *ctx, const plk_r1cs *r, const void *witness_dev, uint64_t n,
                                   int32_t *valid, uint64_t *bad_out /* may be NULL */, void *stream);
/* tracing hook: HIP-event times of the last plk_r1cs_check_witness* on this context, milliseconds: [0] short LCs, [1] long LCs,
 * [2] verdict kernel, [3] the three together with the memsets between them.  Recorded only while plk_set_kernel_timing is on.  */
int32_t plk_r1cs_last_kernel_ms(plk_ctx *ctx, float out_ms[4]);
int32_t plk_validate_witness(plk_ctx *ctx, const plk_setup *s, const plk_circuit *c, int32_t *valid, uint64_t *bad_row /* may be NULL */);

/* ---- one setup, a stream of witnesses: load_witness_from_array (src/reader.rs:119-175) on the GPU, and SetupForProver::prove
 *      (src/plonk.rs:132-159) / validate_witness (:127-129) for a witness that arrives WITHOUT its circuit.  A plk_circuit is the R1CS plus one
 *      witness; a proving service holds one circuit (one plk_setup) and receives a witness per request, and of the circuit the prover reads
 *      nothing but num_variables and the witness once the setup exists.
 *
 *   plk_fr_decode_dev / plk_fr_encode_dev: the two kernels on device pointers (16-byte aligned, else PLK_ERR_ARG), ordered on `stream` like every
 *                _dev call.  decode: n x 32 bytes, each a little-endian canonical integer (the .wtns payload, repr.read_le + Fr::from_repr,
 *                src/reader.rs:169-173) -> n plk_fr in Montgomery form.  It returns its verdict, so it waits for `stream`: an element >= r is
 *                PLK_ERR_FORMAT "read witness failed: not in field", *bad_out = the LOWEST refused index and fr_dev holds zero at every refused
 *                index; else *bad_out = UINT64_MAX.  One decode at a time per context.  encode: the inverse; limbs >= r (never a value this
 *                library made) are encoded after one reduction.
 *   plk_wtns_decode: the whole .wtns file in host memory (pageable is fine) -> fr_dev[0, n).  The container checks are parse_wtns_bin's
 *                (plk_circuit_load's), in its order and with its words — "invalid file header", "unsupported file version", "invalid num
 *                sections", "invalid section type", "invalid section len", "invalid field byte size", "invalid curve prime", "invalid witness
 *                section size", "read witness failed: truncated" — all PLK_ERR_FORMAT, made on the host before the context is read.  *n_out =
 *                elements in the file; fr_dev == NULL only reports it.  cap < n: PLK_ERR_ARG.  The payload starts at byte 76 of the file, which
 *                is not 16-byte aligned: it is copied to the context's staging arena (grows only; the arena of plk_srs_load_key) and decoded
 *                from there, nothing is allocated per call once the arena has grown.  A refused element: as plk_fr_decode_dev.  Blocks.
 *   plk_prove_witness / _witness_dev / _wtns: the bytes plk_prove writes for a plk_circuit that holds the same witness, for the circuit the
 *                setup was prepared from.  n >= num_variables of that circuit; extra elements are ignored (plk_prove_wtns still range-checks
 *                every element of the file), fewer is PLK_ERR_ARG "... the witness does not match the prepared setup".  witness[0] is not read
 *                (wire 0 is zeroed on the device, as in plk_prove); the public inputs are witness[1 .. num_inputs], which the _dev and _wtns
 *                calls copy back before the transcript starts.  Host and _dev: an element of witness[1, num_variables) that is not a canonical
 *                residue is PLK_ERR_ARG, "... wire <lowest such wire> holds an element that is not a canonical residue (limbs >= r)" (the
 *                words of plk_r1cs_check_witness; a kernel finds it).  plk_prove_wtns: the container as plk_wtns_decode, and the decode
 *                kernel's range check is that check (PLK_ERR_FORMAT, *bad_out = lowest refused element, UINT64_MAX otherwise).  A setup from
 *                plk_setup_from_polynomials, a setup not on the device, a commitment in flight, a key too small, an unsatisfying witness
 *                (PLK_ERR_UNSAT, no proof bytes): plk_prove's codes and words under the entry point's own name.  The host vector is never
 *                page-locked.  _dev reads witness_dev[0, num_variables) (16-byte aligned) ordered after the work already enqueued on `stream`
 *                (NULL: the context's stream), blocks like plk_prove and keeps no reference once it returns.  plk_prove_timings ([0] is the
 *                witness upload / decode) and plk_prove_trace describe these proofs as any other.
 *   plk_validate_witness_dev: plk_validate_witness's verdict and bad_row for a device witness (same length, alignment, ordering and canonical
 *                rules as plk_prove_witness_dev).                                                                                            */
int32_t plk_fr_decode_dev(plk_ctx *ctx, const void *bytes_dev, uint64_t n, void *fr_dev, uint64_t *bad_out /* may be NULL */, void *stream);
int32_t plk_fr_encode_dev(plk_ctx *ctx, const void *fr_dev, uint64_t n, void *bytes_dev, void *stream);
/* load_witness_from_array (src/reader.rs:119-175) straight into HBM */
int32_t plk_wtns_decode(plk_ctx *ctx, const uint8_t *data, uint64_t len, void *fr_dev, uint64_t cap, uint64_t *n_out,
                        uint64_t *bad_out /* may be NULL */, void *stream);
/* SetupForProver::prove (src/plonk.rs:132-159) for the next witness of the circuit the setup was prepared from */
int32_t plk_prove_witness(plk_ctx *ctx, const plk_setup *s, const plk_fr *witness_host, uint64_t n, uint8_t *proof_out, uint64_t cap, uint64_t *len);
int32_t plk_prove_witness_dev(plk_ctx *ctx, const plk_setup *s, const void *witness_dev, uint64_t n, uint8_t *proof_out, uint64_t cap, uint64_t *len,
                              void *stream);
int32_t plk_prove_wtns(plk_ctx *ctx, const plk_setup *s, const uint8_t *wtns, uint64_t wtns_len, uint8_t *proof_out, uint64_t cap, uint64_t *len,
                       uint64_t *bad_out /* may be NULL */);
/* SetupForProver::validate_witness (src/plonk.rs:127-129) for a device witness */
int32_t plk_validate_witness_dev(plk_ctx *ctx, const plk_setup *s, const void *witness_dev, uint64_t n, int32_t *valid,
                                 uint64_t *bad_row /* may be NULL */, void *stream);

/* ---- assembled input: SetupPolynomials and the wire columns of bellman's own synthesis (src/plonk.rs:50-55,104,152-159) */
/* plonkit's SetupForProver holds bellman's SetupPolynomials (src/plonk.rs:50-55, built by setup() at :104) and prove_by_steps takes
 * that setup plus the circuit bellman has already synthesised (:152-159).  These entry points take the same data one level below
 * plk_circuit_load: no transpiler of this library is involved, so a circuit proved this way gets the proof bellman's own assembly
 * defines.
 *   Layout.      Every vector is an array of plk_fr, Montgomery form, byte-identical to ff_ce's Fr.  The order is the one vk.bin stores the
 *                commitments in: selectors q_a q_b q_c q_d q_m q_const, then the next-step selector q_d_next, then sigma_1..sigma_4.
 *   Domain.      N = n + 1 must be a power of two with log2 N + 2 <= 28; otherwise PLK_ERR_SIZE "setup power of two is not in the
 *                correct range" (plk_setup_prepare's code and words).
 *   Length.      Coefficient form (flags = 0): 1 <= len <= N monomial coefficients per vector, zero-extended to N.  Value form
 *                (PLK_POLY_VALUES): len == N evaluations on <omega_N> in row order.  Otherwise PLK_ERR_ARG.  num_inputs <= n.
 *   Rows.        num_inputs <= rows <= N (else PLK_ERR_ARG); columns are zero-extended to N.  Public input i is column a at row i,
 *                the row whose gate is q_a = -1 in plk_setup_prepare's setup and where plk_prove takes it from: there is no separate
 *                inputs argument that could disagree with the columns.
 *   Checks.      Any selector, sigma or column element that is not a canonical residue (limbs >= r): PLK_ERR_ARG.  A row that fails
 *                the width-4 gate equation q_a a + q_b b + q_c c + q_d d + q_m a b + q_const + q_d_next d_next + PI = 0:
 *                PLK_ERR_UNSAT, "must satisfy: ... at row <lowest failing row> ..." (src/plonk.rs:137).  A permutation argument
 *                that does not close (prod of numerators != prod of denominators at the transcript's beta, gamma — the columns
 *                break the copy constraints of sigma): PLK_ERR_UNSAT, "copy constraints: ...".  No proof bytes in either case.
 *                Key too small: PLK_ERR_SRS, as plk_prove.
 *   Both kinds of setup.  plk_prove on a setup from plk_setup_from_polynomials is PLK_ERR_ARG (it has no gate structure);
 *                plk_prove_assembled* work on a plk_setup_prepare setup too.  plk_setup_write_vk, plk_setup_upload (a no-op: the
 *                setup is resident when the call returns), plk_setup_domain_size and plk_setup_free work on both, and
 *                plk_prove_timings / plk_prove_trace describe an assembled proof as any other ([0] is the column upload there).
 *   Host columns are never page-locked: they are copied as pageable memory.  The _dev variant reads columns_dev[j][0, rows) on the
 *   device, ordered after the work already enqueued on `stream` (NULL: the context's stream, see the conventions above); it blocks
 *   like plk_prove and keeps no reference to the columns once it returns.                                                         */
#define PLK_POLY_VALUES 1u    /* vectors are evaluations on <omega_N> in row order, not monomial coefficients */
/* SetupPolynomials<Bn256, PlonkCsWidth4WithNextStepParams> -> a resident setup (src/plonk.rs:50-55,104): 11 uploads, 11 NTT(N) */
int32_t plk_setup_from_polynomials(plk_ctx *ctx, uint64_t n, uint64_t num_inputs,
                                   const plk_fr *const selectors[6],      /* q_a q_b q_c q_d q_m q_const */
                                   const plk_fr *next_step_selector,      /* q_d_next                    */
                                   const plk_fr *const sigmas[4], uint64_t len, uint32_t flags, plk_setup **out);
/* prove_by_steps from the assembled columns a, b, c, d (src/plonk.rs:152-159) -> proof.bin bytes (Proof::write) */
int32_t plk_prove_assembled(plk_ctx *ctx, const plk_setup *s, const plk_fr *const columns[4], uint64_t rows,
                            uint8_t *proof_out, uint64_t cap, uint64_t *len);
int32_t plk_prove_assembled_dev(plk_ctx *ctx, const plk_setup *s, const void *const columns_dev[4], uint64_t rows,
                                uint8_t *proof_out, uint64_t cap, uint64_t *len, void *stream);

/* ---- the polynomial helpers of rounds 2, 4 and 5 on their own (bellman_ce::plonk::polynomials / better_cs::prover, reached
 *      from prove_by_steps src/plonk.rs:152-159): Polynomial::evaluate_at, the division by (x - z) behind the two opening
 *      proofs ((p(x) - p(z)) / (x - z), n coefficients, the top one zero), and the permutation grand product
 *      z_0 = 1, z_{i+1} = z_i * prod_j (w_j + beta k_j omega^i + gamma) / (w_j + beta sigma_j + gamma)  (SURVEY.md A.4 round 2;
 *      k = 1, 5, 7, 10; no per-element inversion: prefix x suffix products and one host inversion).  Device vectors, N = 2^log_n.
 *      plk_poly_evaluate_at_dev at z = 0 returns c_0.  plk_poly_divide_by_linear_dev refuses z = 0 with PLK_ERR_ARG (its schedule
 *      multiplies by powers of 1/z; the quotient by x is a shift the caller can do).  plk_permutation_grand_product_dev returns
 *      PLK_ERR_UNSAT ("grand product denominator vanished") when w_j[i] + beta sigma_j[i] + gamma = 0 for some j and some row i of
 *      the N, the last row included; z_values_dev is unspecified then and the context stays usable.
 *      plk_setup_permutation_dev is the copy-constraint permutation of plk_setup_prepare on its own (the setup calls the same code):
 *      vars_dev[j] holds the 2^log_n uint32 variable ids of column j (a, b, c, d); id 0 is the dummy variable; every id is < num_vars —
 *      the CALLER guarantees that, nothing checks it on the device (num_vars decides how many bits are sorted).  All occurrences of
 *      an id, in row-major order (row by row, a to d inside a row), map each to the next and the last to the first; id 0 and single
 *      occurrences keep the identity.  index_dev (may be NULL) receives idx[col * n + row] = col' << 30 | row', sigmas_dev (may be
 *      NULL, not both) the four columns k_col' * omega^row' in Montgomery form.  log_n <= 26, the largest setup (SETUP_MAX_POW2).
 *      PLK_ERR_ARG: a null pointer, log_n > 26, num_vars = 0, both outputs NULL.  Blocks until the outputs are written. */
int32_t plk_poly_evaluate_at_dev(plk_ctx *ctx, const void *coeffs_dev, uint64_t n, const plk_fr *z, plk_fr *out, void *stream);
int32_t plk_poly_divide_by_linear_dev(plk_ctx *ctx, const void *coeffs_dev, uint64_t n, const plk_fr *z, void *quotient_dev, void *stream);
int32_t plk_permutation_grand_product_dev(plk_ctx *ctx, const void *const wires_dev[4], const void *const sigmas_dev[4], const plk_fr *beta, const plk_fr *gamma,
                                          uint32_t log_n, void *z_values_dev, void *stream);
int32_t plk_setup_permutation_dev(plk_ctx *ctx, const void *const vars_dev[4], uint32_t log_n, uint64_t num_vars,
                                  void *index_dev /* 4 * 2^log_n uint32, may be NULL */,
                                  void *const sigmas_dev[4] /* 2^log_n plk_fr each, may be NULL */, void *stream);

/* ---- which copy constraint is broken: the exact checks behind "copy constraints: the permutation argument does not close" of
 *      plk_prove_assembled* (prove_by_steps on a caller's sigma and columns, src/plonk.rs:152-159; bellman reports nothing here).
 *      No key, no transcript, no beta / gamma: nothing below is probabilistic.
 *      plk_sigma_decode_dev is the inverse of the sigmas_dev output of plk_setup_permutation_dev: every value x of the four columns
 *      that equals k_c * omega_N^i (k = 1, 5, 7, 10, i < N = 2^log_n, Montgomery form) gives idx[col * N + row] = c << 30 | i, every
 *      other value — 0, another coset, an element of order 2N, limbs >= r — gives 0xFFFFFFFF.  The discrete logarithm is exact
 *      (2-power group order, one bit per step); a value counts as decoded only if the label recomputed from (c, i) equals it limb
 *      for limb.  *bad_key (may be NULL) receives row * 4 + col of the lowest refused cell, UINT64_MAX if none.  1 <= log_n <= 26;
 *      a null pointer or another log_n is PLK_ERR_ARG.  Blocks until the outputs are written.
 *      The three checks return PLK_OK whenever they reached a verdict, which is out->kind (the convention of plk_validate_witness);
 *      PLK_ERR_* is for bad arguments and HIP errors only.  "Lowest" is by row * 4 + col everywhere: row first, then a, b, c, d inside
 *      the row — the order plk_setup_permutation_dev links occurrences in and the gate check counts rows in.
 *      plk_setup_check_permutation looks at the setup's sigma alone (kinds 0, 1, 2): is every value a cell label, and is every cell
 *      the image of some cell.  plk_check_copies* run those two first (kinds 1 and 2 win) and then compare every cell's value with
 *      that of its image (kind 3).  rows and canonicity as plk_prove_assembled*: num_inputs <= rows <= N, zero beyond rows, an element
 *      >= r is PLK_ERR_ARG.  Both kinds of setup.  When the permutation argument of plk_prove_assembled* does not close, the same
 *      localisation runs on the columns already on the device and its finding is appended to the message:
 *      "...; first broken copy: cell b[17] and its image c[3] hold different values", "...; sigma is not a permutation: cell a[5] is
 *      the image of no cell", "...; sigma is not a permutation: its value at cell d[2] is not a cell label".  A proof that succeeds
 *      launches none of this.                                                                                                        */
typedef struct { uint32_t kind; uint32_t col, row; uint32_t col2, row2; } plk_copy_report;
#define PLK_COPY_OK            0u
#define PLK_COPY_NOT_A_LABEL   1u   /* sigma_col(omega^row) is no k_c * omega^i: (col,row) = lowest such cell                        */
#define PLK_COPY_NOT_BIJECTIVE 2u   /* every value decodes, but (col,row) = lowest cell that is the image of no cell                 */
#define PLK_COPY_BROKEN        3u   /* (col,row) = lowest cell whose value differs from that of its image (col2,row2)                */
int32_t plk_sigma_decode_dev(plk_ctx *ctx, const void *const sigmas_dev[4], uint32_t log_n,
                             void *index_dev /* 4 * 2^log_n uint32, the layout of plk_setup_permutation_dev */,
                             uint64_t *bad_key /* may be NULL */, void *stream);
int32_t plk_setup_check_permutation(plk_ctx *ctx, const plk_setup *s, plk_copy_report *out);
int32_t plk_check_copies(plk_ctx *ctx, const plk_setup *s, const plk_fr *const columns[4], uint64_t rows, plk_copy_report *out);
int32_t plk_check_copies_dev(plk_ctx *ctx, const plk_setup *s, const void *const columns_dev[4], uint64_t rows, plk_copy_report *out, void *stream);

/* ---- KZG openings on their own (kzg.hip): bellman's kate_commitment beyond the commitments (the module src/plonk.rs:4 takes `Crs` from) —
 *      commit_using_monomials / commit_using_values, open_from_monomials / open_from_values and is_valid_opening.  The prover does all of
 *      this inside round 5; here a caller opens a commitment at a point, from coefficients or from the values on the domain, and checks
 *      openings.  Scalars are Montgomery plk_fr below r, points plk_g1_affine with (0, 0) as infinity; polynomials live in device memory,
 *      16-byte aligned, and are never written (the one exception: a quotient written over its own input where that is said to be allowed).
 *      N = 2^log_n, omega = the library's root of unity of that order (plk_ntt_dev's).
 *
 *   plk_poly_evaluate_values_at_dev.  f(z) from the N values f(omega^i), 1 <= log_n <= 28, by the barycentric formula
 *                f(z) = (z^N - 1) / N * sum_i f_i omega^i / (z - omega^i); z = omega^k returns f_k exactly, read from the array.  No transform,
 *                no per-element inversion: per-element denominators from the context's omega table, prefix x suffix products (the scans of
 *                the grand product) and ONE host inversion.  Blocks, like plk_poly_evaluate_at_dev.  No host pass over the N elements.
 *   plk_poly_divide_values_by_linear_dev.  The N values of q = (f - y) / (x - z): q_i = (f_i - y) / (omega^i - z) for omega^i != z; for
 *                z = omega^k position k holds q(omega^k) = sum_{i != k} (f_i - y) omega^i / (z (z - omega^i)), the value there of the
 *                polynomial quotient of degree < N - 1.  y == NULL: f(z), computed as above.  A caller's y is taken on trust outside the
 *                domain, as open_from_values takes its expected value; inside the domain y != f_k is PLK_ERR_ARG (no polynomial quotient
 *                exists).  The output may be the input.  Waits before it returns, as plk_poly_divide_by_linear_dev.
 *   plk_kzg_commit_dev.  commit_using_monomials: exactly plk_msm_g1_batch_dev at offset 0 (count <= 8).  With PLK_KZG_VALUES the vectors are
 *                values and are summed against the Lagrange-form slot (commit_using_values); no such key, or one whose size is not n:
 *                PLK_ERR_SRS, "Lagrange-form key has a different size than the circuit's domain" (the prover's words).
 *   plk_kzg_open_dev.  y_j = f_j(z) into evals[j], F = sum_j v^j f_j, Y = sum_j v^j y_j, *proof = commit((F - Y) / (x - z)): the shape of
 *                round 5.  v may be NULL when count == 1.  Without flags the inputs are coefficients, 1 <= n <= plk_srs_size: the linear
 *                combination, division and evaluation kernels of the prover; z = 0 works here (the quotient is the combination moved down
 *                by one coefficient, y = c_0) while plk_poly_divide_by_linear_dev keeps its refusal.  With PLK_KZG_VALUES n is the
 *                Lagrange-form key's size (else PLK_ERR_SRS as above), the quotient is formed in values by the kernels of the two calls above
 *                and committed against the Lagrange-form slot: no transform is launched, and the proof is the same point, bit for bit, as
 *                the coefficient route gives for the interpolated polynomials.  Blocks.  A commitment in flight on the context: PLK_ERR_ARG,
 *                as the other blocking calls.  Null pointers, count outside 1..8, n = 0, unknown flags, a scalar >= r: PLK_ERR_ARG.
 *                Scratch (3 N x 32 B in values, 2 n x 32 B + 2 MiB in coefficients) grows only; a call that grew it past 64 MiB frees it
 *                before it returns.  Single-GPU: the commitment is plk_msm_g1_dev's, a sharded key commits its own slice only.
 *   plk_kzg_verify.  is_valid_opening, pure CPU, no context.  C = sum_j v^j C_j, Y = sum_j v^j y_j; *valid = 1 exactly when
 *                e(C - Y G + z pi, g2[0]) e(-pi, g2[1]) == 1, through plk_pairing_check (its G2 decoding, its refusals, its words).
 *                Infinity is a legal commitment (the zero polynomial) and a legal proof (a constant).  A point off the curve, a coordinate
 *                >= q, a scalar >= r, count outside 1..8, v == NULL with count > 1: PLK_ERR_ARG.
 *   plk_kzg_verify_many_dev.  n independent single-polynomial openings in device memory: commitments, z, evaluations, proofs (16-byte
 *                aligned) and one verdict byte each (any alignment).  Ordered on `stream`, does not wait.  NO COUNTERPART IN THE REFERENCE.
 *                One lane per opening range-checks the two scalars, curve-checks the two points and forms A_i = C_i + z_i pi_i + (-y_i) G
 *                and B_i = -pi_i (two GLV multiplications of g1_mul_dev.h); plk_pairing_check_many_dev's kernel then decides every
 *                e(A_i, Q_0) e(B_i, Q_1) == 1 on its own.  Verdict i = 1 / 0 / PLK_VERDICT_MALFORMED is what plk_kzg_verify says about
 *                opening i (malformed: where it returns PLK_ERR_ARG for the opening's own data): no random combination across openings, the
 *                rule of plk_verify_many; a malformed entry does not touch its neighbours.  g2 as plk_pairing_check_many_dev (a pair the
 *                context did not see last waits for the stream once).  n == 0 launches nothing.  Memory and order as plk_verify_many_dev:
 *                274 B per opening (at most 2^16 per pass) in a grows-only buffer of its own outside the staging arena, kernels on the
 *                context's stream between two events.
 *                BREAK-EVEN (one MI355X, profiles/kzg_open.txt): a call costs ~88 ms whatever the batch up to a few thousand openings (one
 *                pairing lane per opening), a plk_kzg_verify 12.5 ms.  Measured at 1 / 256 / 4096 openings: 92 / 89 / 89 ms against 13 / 198 /
 *                3218 ms for a loop of plk_kzg_verify on 16 host threads — 256 is the first measured size at which this call wins (the
 *                figures cross near 110).  Below that, prefer plk_kzg_verify on host threads.                                          */
#define PLK_KZG_VALUES 1u     /* the vectors are values on <omega_N>, committed against the Lagrange-form key */
int32_t plk_poly_evaluate_values_at_dev(plk_ctx *ctx, const void *values_dev, uint32_t log_n, const plk_fr *z, plk_fr *out, void *stream);
int32_t plk_poly_divide_values_by_linear_dev(plk_ctx *ctx, const void *values_dev, uint32_t log_n, const plk_fr *z, const plk_fr *y /* NULL: f(z) */,
                                             void *quotient_values_dev, void *stream);
int32_t plk_kzg_commit_dev(plk_ctx *ctx, const void *const *polys_dev, uint32_t count, uint64_t n, uint32_t flags, plk_g1_affine *out, void *stream);
int32_t plk_kzg_open_dev(plk_ctx *ctx, const void *const *polys_dev, uint32_t count, uint64_t n, const plk_fr *z, const plk_fr *v /* may be NULL when count == 1 */,
                         uint32_t flags, plk_fr *evals, plk_g1_affine *proof, void *stream);
int32_t plk_kzg_verify(const plk_g1_affine *commitments, uint32_t count, const plk_fr *z, const plk_fr *evals, const plk_fr *v /* may be NULL when count == 1 */,
                       const plk_g1_affine *proof, const uint8_t g2[256], int32_t *valid);
int32_t plk_kzg_verify_many_dev(plk_ctx *ctx, const void *commitments_dev, const void *z_dev, const void *evals_dev, const void *proofs_dev, uint64_t n,
                                const uint8_t g2[256], void *verdict_dev, void *stream);
/*   plk_kzg_open_all_dev.  The openings at ALL N = 2^log_n points of the domain in one pass (kzg_all.hip, Feist-Khovratovich): proofs_dev[i]
 *                is, byte for byte, the proof plk_kzg_open_dev returns for the same polynomial at z = omega^i.  NO COUNTERPART IN THE
 *                REFERENCE (kate_commitment opens one point per call).  With h_k = sum_j f_{k+1+j} s_j (s_j the key's points) the proofs
 *                are DFT_N(h), and h is one cyclic correlation of length 2N: a scalar NTT of the coefficients at 2N, a point-wise
 *                G1 x Fr product with the key's transform (2N multiplications of g1_mul_dev.h), the inverse G1 transform at 2N, the
 *                forward one at N, one conversion to affine.  poly_dev: N coefficients, or with PLK_KZG_VALUES the N values on the domain
 *                (one inverse NTT into scratch first; this route reads NO Lagrange-form key); never written.  evals_dev, if not NULL,
 *                receives f(omega^i) (one more NTT; with PLK_KZG_VALUES a copy of the input); it must not be poly_dev.  0 <= log_n <= 25
 *                (PLK_ERR_SIZE above; log_n = 0 gives the point at infinity); key points 0 .. N - 2 are read: PLK_ERR_SRS when fewer than
 *                N - 1 are resident.  A borrowed or lent key (plk_srs_set_dev, plk_ctx_share_srs) will do.  Single-GPU (a context with a
 *                commit shard: PLK_ERR_ARG), 16-byte aligned pointers, no commitment in flight (the transforms of g1ntt.hip share their
 *                refusals).  Blocks.  Memory: the key's transform, 2N x 144 B, is built by the first call for a size (or by
 *                plk_kzg_open_all_prepare) and kept by the calling context until its key changes or another size is asked for; scratch of
 *                2N x 176 B (+ N x 32 B in values) beside it grows only, and a call that grew it past 64 MiB frees it before it returns.
 *                MEASURED (one MI355X, profiles/kzg_open_all.txt): 2^12 / 2^16 / 2^20 points 22 / 31 / 447 ms with the key's transform kept,
 *                33 / 46 / 727 ms when the call has to build it; the loop of 4096 plk_kzg_open_dev calls at 2^12 takes 1290 ms.
 *   plk_kzg_open_all_prepare.  Builds and keeps the key's transform for 2^log_n; optional.  The same refusals.  Blocks.
 *   plk_kzg_open_all_last_ms.  Device-event times of the last call while plk_set_kernel_timing is on: the key's transform (about 0 when it
 *                was cached), the scalar NTTs, the point-wise product, the inverse transform, the forward transform with the conversion.
 *   plk_g1_ntt_dev.  The transform of plk_g1_intt over 2^log_n affine points in device memory (64 B each, (0, 0) = infinity), in either
 *                direction: inverse != 0 is plk_g1_intt bit for bit (omega^-1, 1 / N); inverse == 0 is out[i] = sum_j omega^(i j) in[j],
 *                no scaling.  log_n <= 26, no commitment in flight (the scratch is slot 0's).  Ordered on `stream`, does not wait; out_dev
 *                may be in_dev.
 *   plk_kzg_open_all_batch_dev.  plk_kzg_open_all_dev for `count` polynomials under the one key in one pass: a holder of many columns (a
 *                data-availability holder, the cached quotients of a lookup argument) pays the stage launches of one.  polys_dev: count
 *                polynomials back to back, N = 2^log_n plk_fr each (coefficients, or values with PLK_KZG_VALUES); never written.
 *                proofs_dev[b N + i] is, byte for byte, what plk_kzg_open_all_dev writes at [i] for polynomial b; evals_dev[b N + i], if
 *                not NULL, is f_b(omega^i); nothing beyond count x N entries is written.  count >= 1 (0: PLK_ERR_ARG), log_n <= 25 and
 *                count x 2^(log_n + 1) <= 2^26 (PLK_ERR_SIZE above, nothing allocated: g1ntt's limit for a whole launch, every flattened
 *                index inside 32 bits); every other refusal of plk_kzg_open_all_dev in its order, under this function's name.  log_n = 0:
 *                count points at infinity, the evals copied from the input.  The key's transform is THE SAME kept one: either entry point
 *                (or plk_kzg_open_all_prepare) builds it for both, a change of the key voids it for both.  Scratch: count x 2N x 176 B
 *                (+ count x N x 32 B in values), the same buffer and rule as the single call's.  Blocks; plk_kzg_open_all_last_ms reports
 *                its five parts.  Every G1 stage launch covers all count transforms (the polynomial is the slow index, the key's
 *                transform is read at m mod 2N); the scalar NTTs run one polynomial at a time.
 *                MEASURED (one MI355X, profiles/kzg_open_all_batch.txt, the key's transform kept): at 2^12, 1 / 4 / 16 / 64 polynomials take
 *                22.4 / 22.9 / 25.0 / 76.7 ms where the loop of single calls takes 22.3 / 89.2 / 357 / 1428 ms (16: 14.3 x, 64: 18.6 x);
 *                at 2^16, where one polynomial already fills the chip, 1 / 4 / 16 take 31.5 / 93.1 / 364 ms against 31.4 / 125 / 504 (1.4 x).
 *   plk_g1_ntt_batch_dev.  plk_g1_ntt_dev over `count` arrays of 2^log_n affine points back to back, in either direction: row b of the
 *                output equals plk_g1_ntt_dev of row b byte for byte.  count >= 1 (0: PLK_ERR_ARG), count << log_n <= 2^26
 *                (PLK_ERR_SIZE).  Slot 0's scratch: the refusals of plk_g1_ntt_dev.  Ordered on `stream`, does not wait; out_dev may be
 *                in_dev.                                                                                                                 */
int32_t plk_kzg_open_all_prepare(plk_ctx *ctx, uint32_t log_n);
int32_t plk_kzg_open_all_dev(plk_ctx *ctx, const void *poly_dev, uint32_t log_n, uint32_t flags /* 0 | PLK_KZG_VALUES */,
                             void *proofs_dev /* 2^log_n affine points */, void *evals_dev /* may be NULL: f(omega^i) */, void *stream);
int32_t plk_kzg_open_all_last_ms(plk_ctx *ctx, float out_ms[5]);
int32_t plk_g1_ntt_dev(plk_ctx *ctx, const void *in_dev, uint32_t log_n, int32_t inverse, void *out_dev, void *stream);
int32_t plk_kzg_open_all_batch_dev(plk_ctx *ctx, const void *polys_dev, uint32_t count, uint32_t log_n, uint32_t flags /* 0 | PLK_KZG_VALUES */,
                                   void *proofs_dev /* count x 2^log_n affine points */, void *evals_dev /* may be NULL */, void *stream);
int32_t plk_g1_ntt_batch_dev(plk_ctx *ctx, const void *in_dev, uint32_t count, uint32_t log_n, int32_t inverse, void *out_dev, void *stream);
/*   Many polynomials at several points with a proof of two points (kzg_multi.hip; Boneh-Drake-Fisch-Gabizon 2020, the scheme that needs
 *   only [tau]_2).  NO COUNTERPART IN THE REFERENCE: kate_commitment opens at one point per call.  f_0 .. f_{m-1} have n coefficients each,
 *   t_0 .. t_{p-1} are distinct points, and bit j of sets[i] says that f_i is opened at t_j (S_i; T = all p points).  No set is empty, no
 *   bit at or above p is set, every point belongs to some set.  Z_A(x) = prod_{a in A} (x - a), r_i = the polynomial of degree < |S_i| that
 *   agrees with f_i on S_i, w_ij = 1 / prod_{l in S_i, l != j} (t_j - t_l), gamma^i is indexed by the polynomial's position.
 *       W  = commit(h),  h = sum_i gamma^i (f_i - r_i) / Z_{S_i} = sum_j D_{t_j}[ sum_{i: j in S_i} gamma^i w_ij f_i ],  D_t[g] = (g - g(t)) / (x - t)
 *       u  = the caller's challenge, drawn after W
 *       W' = commit(L / (x - u)),  L = sum_i c_i (f_i - r_i(u)) - Z_T(u) h,  c_i = gamma^i Z_{T \ S_i}(u)
 *   and an opening is valid exactly when e(F + u W', g2[0]) e(-W', g2[1]) == 1 with F = sum_i c_i (C_i - r_i(u) G) - Z_T(u) W.
 *
 *   plk_poly_quotient_multi_dev.  The operator behind both quotients, as a call of its own (what the tests hold against the definition):
 *                out[k] = sum_j sum_{l > k} G_j[l] t_j^(l-k-1),  G_j[l] = sum_i coef[i * npoints + j] f_i[l],  k < n; out[n-1] = 0.
 *                That is sum_j D_{t_j}[G_j].  count 1..64, npoints 1..8, 1 <= n <= 2^28; coef and points are host arrays of scalars
 *                below r; a zero entry of coef costs no product.  Every polynomial is read once per pass for all points (two passes over
 *                tiles of 2048 coefficients and a carry between them: (2 count + 1) x 32 n bytes), no npoints x n intermediate exists, no
 *                inverse is taken, and t_j = 0 is an ordinary point (the shifted combination).  The points need not be distinct here.
 *                The same pointer may appear twice among the inputs; out_dev is none of them (PLK_ERR_ARG).  Blocks.
 *   plk_kzg_open_multi_dev.  The prover above.  Inputs are COEFFICIENTS, 1 <= n <= plk_srs_size, n <= 2^28, count 1..32, npoints 1..8; there
 *                is no flags argument: a holder of values calls plk_kzg_open_multi_values_dev.  evals[i * npoints + j] = f_i(t_j) for j in S_i and
 *                zero elsewhere (the evaluation kernel of the prover, 12 pairs per launch); the two points do not depend on them.
 *                `challenge` is called ONCE, on the calling thread, after W has reached the host, and not at all when the call fails
 *                earlier; it writes u.  A non-zero return: PLK_ERR_IO, the message names the callback and its return value; u >= r:
 *                PLK_ERR_ARG; the context stays usable after either.  Any u below r is legal, 0 and the points included, and so is any
 *                point below r.  *u_out receives u, proof[0] = W, proof[1] = W'.  Polynomials are never written; the same pointer may
 *                appear twice.  PLK_ERR_ARG: null pointers, counts out of range, duplicate points, an empty set, a set bit at or above
 *                npoints, a point no set uses, a scalar >= r, pointers not 16-byte aligned, a commitment in flight, a context with a
 *                commit shard (single-GPU).  PLK_ERR_SRS: no key resident, or the key is shorter than n.  Blocks.  Scratch (h, one value
 *                per tile and point, the matrix, the power tables of the points: about n x 32 B + 8.3 MiB) lives in the opening calls'
 *                buffer: grows only, and a call that grew it past 64 MiB frees it before it returns.
 *   plk_kzg_verify_multi.  The verifier above, pure CPU, no context: count + 3 scalar multiplications and plk_pairing_check (its G2
 *                decoding, its refusals, its words).  evals is count x npoints, entries outside a set are not read.  Infinity is a legal
 *                commitment and a legal W or W'.  The refusals of plk_kzg_verify and those of the sets above: PLK_ERR_ARG.  count 1..32.
 *   plk_kzg_open_multi_last_ms.  Device-event times of the last plk_kzg_open_multi_dev while plk_set_kernel_timing is on: the evaluations,
 *                the quotient h, the commitment W, the second quotient with the commitment W'.                                            */
typedef int32_t (*plk_kzg_challenge_fn)(void *user, const plk_g1_affine *w, plk_fr *u_out);   /* 0 = success */
int32_t plk_poly_quotient_multi_dev(plk_ctx *ctx, const void *const *polys_dev, uint32_t count /* 1..64 */, uint64_t n,
                                    const plk_fr *points, uint32_t npoints /* 1..8 */, const plk_fr *coef /* count x npoints, row-major */,
                                    void *out_dev /* n elements; not one of the inputs */, void *stream);
int32_t plk_kzg_open_multi_dev(plk_ctx *ctx, const void *const *polys_dev, uint32_t count /* 1..32 */, uint64_t n,
                               const plk_fr *points, uint32_t npoints /* 1..8 */, const uint32_t *sets /* count masks */,
                               const plk_fr *gamma, plk_kzg_challenge_fn challenge, void *user,
                               plk_fr *evals /* count x npoints; entries outside a set are written as zero */,
                               plk_fr *u_out, plk_g1_affine proof[2] /* W, W' */, void *stream);
int32_t plk_kzg_verify_multi(const plk_g1_affine *commitments, uint32_t count, const plk_fr *points, uint32_t npoints,
                             const uint32_t *sets, const plk_fr *evals /* count x npoints; entries outside a set are not read */,
                             const plk_fr *gamma, const plk_fr *u, const plk_g1_affine proof[2],
                             const uint8_t g2[256], int32_t *valid);
int32_t plk_kzg_open_multi_last_ms(plk_ctx *ctx, float out_ms[4]);
/*   The same openings FROM VALUES ON THE DOMAIN (kzg_multi_values.hip): values_dev[i] holds the N = 2^log_n values f_i(omega^k), the layout
 *   PLK_KZG_VALUES means elsewhere; no transform runs and no coefficient copy exists.  NO COUNTERPART IN THE REFERENCE.  1 <= log_n <= 28.
 *   A point may lie on the domain (t_j = omega^k, decided by t_j^N = 1): the evaluation is then read from the arrays and position k of a
 *   quotient takes the value of the polynomial quotient there, as plk_poly_divide_values_by_linear_dev has it.  ONE inversion serves all
 *   points of a call (a product scan over prod_j (omega^x - t_j)); working memory is two vectors, the output and one partial sum per
 *   (polynomial, point) pair and tile of 2048, whatever the number of polynomials.
 *
 *   plk_kzg_open_multi_values_dev.  plk_kzg_open_multi_dev for a holder of values: evals, *u_out, proof[0] = W and proof[1] = W' are byte
 *                for byte what that call returns for the coefficients of the same polynomials with n = N under the same key, points, sets,
 *                gamma and callback, so plk_kzg_verify_multi and plk_kzg_verify_multi_many_dev take them unchanged.  The commitments go
 *                against the LAGRANGE-FORM key: none resident, or one of another size than N, is PLK_ERR_SRS in the words of
 *                plk_kzg_open_dev's values route.  log_n out of range: PLK_ERR_ARG.  Every other refusal, the callback rules (called once,
 *                on the calling thread, after W has reached the host; non-zero return PLK_ERR_IO; u >= r PLK_ERR_ARG) and the blocking
 *                are plk_kzg_open_multi_dev's, in its words behind this call's name.  u may be any scalar below r: 0, 1, a point of the
 *                domain (the value of the second quotient's numerator at u, known from the evaluations, is then held against the arrays:
 *                a mismatch is PLK_ERR_HIP), one of the t_j.  Inputs are never written; the same pointer may appear twice.
 *   plk_poly_quotient_multi_values_dev.  The operator on its own: out = the N values of sum_j D_{t_j}[sum_i coef[i * npoints + j] f_i]; it
 *                finds the G_j(t_j) itself (the evaluation pass over the pairs with a non-zero coefficient).  count 1..64, npoints 1..8,
 *                the points need not be distinct; out overlaps none of the inputs (PLK_ERR_ARG).  Needs no key.  Blocks.
 *   plk_poly_evaluate_values_multi_dev.  The evaluation pass on its own: evals[i * npoints + j] = f_i(points[j]) for bit j of sets[i], zero
 *                elsewhere; every polynomial is read once for all its points.  count 1..64; a set may be empty, a bit at or above npoints
 *                is PLK_ERR_ARG.  Needs no key.  Blocks.
 *   plk_kzg_open_multi_last_ms reports the last opening of either route.  On the values route: [0] the denominators, the scan pair, the
 *                inversion, k_kml_sums / k_kml_sum_finish and the evaluations' way to the host; [1] the matrix upload and k_kml_quot for h;
 *                [2] the commitment W; [3] the same three steps for u (sums only when u lies on the domain), k_kml_quot<1> over the
 *                count + 1 vectors and the commitment W'.
 *   MEASURED at 2^20 (profiles/kzg_open_multi_values.txt), against count copies, count inverse plk_ntt_dev and
 *                plk_kzg_open_multi_dev: (8 polynomials, 1 point) 3.9 against 4.3 ms, (8, 3) 4.2 against 4.5 ms, (32, 8) 7.2 against 11.6 ms;
 *                the median lies below the other leg's minimum at each.  A caller that already holds coefficients keeps
 *                plk_kzg_open_multi_dev at the two small shapes (3.4 and 3.6 ms without the transforms).                                  */
int32_t plk_kzg_open_multi_values_dev(plk_ctx *ctx, const void *const *values_dev, uint32_t count /* 1..32 */, uint32_t log_n,
                                      const plk_fr *points, uint32_t npoints /* 1..8 */, const uint32_t *sets /* count masks */,
                                      const plk_fr *gamma, plk_kzg_challenge_fn challenge, void *user,
                                      plk_fr *evals /* count x npoints; entries outside a set are written as zero */,
                                      plk_fr *u_out, plk_g1_affine proof[2] /* W, W' */, void *stream);
int32_t plk_poly_quotient_multi_values_dev(plk_ctx *ctx, const void *const *values_dev, uint32_t count /* 1..64 */, uint32_t log_n,
                                           const plk_fr *points, uint32_t npoints /* 1..8 */, const plk_fr *coef /* count x npoints, row-major */,
                                           void *out_values_dev /* 2^log_n elements; not one of the inputs */, void *stream);
int32_t plk_poly_evaluate_values_multi_dev(plk_ctx *ctx, const void *const *values_dev, uint32_t count /* 1..64 */, uint32_t log_n,
                                           const plk_fr *points, uint32_t npoints /* 1..8 */, const uint32_t *sets /* count masks */,
                                           plk_fr *evals /* count x npoints, zero outside the sets */, void *stream);
/*   plk_kzg_verify_multi_many_dev.  n openings of the scheme above in device memory, verified each on its own (kzg_multi_verify.hip).  NO
 *                COUNTERPART IN THE REFERENCE.  ONE SHAPE serves the batch — count, npoints and the sets (a host array) are one protocol's;
 *                per opening the arrays hold count commitments, npoints points, count x npoints evaluations (row-major, as
 *                plk_kzg_verify_multi takes them), gamma, u and the two proof points W, W'.  Verdict i = 1 / 0 / PLK_VERDICT_MALFORMED is
 *                exactly what plk_kzg_verify_multi says about opening i under that shape: no random combination across openings, no
 *                bisection, the rule of plk_verify_many.  Malformed is where it returns PLK_ERR_ARG for the opening's own data: a point off
 *                the curve, a coordinate >= q, gamma, u, a point or an evaluation INSIDE its set >= r, two equal points (decided on the
 *                device: it is a property of one opening).  Evaluations outside a set are not read.  Infinity is a legal commitment, W and
 *                W'.  A malformed opening contributes nothing to the arithmetic and does not touch its neighbours.
 *                What the host refuses, once, from the sets alone (PLK_ERR_ARG, plk_kzg_verify_multi's words): count outside 1..32, npoints
 *                outside 1..8, an empty set, a bit at or above npoints, a point no set uses.  Otherwise as plk_kzg_verify_many_dev: ordered
 *                on `stream`, does not wait; n == 0 launches nothing; pointers 16-byte aligned, the verdict pointer of any alignment;
 *                n <= 2^28 (PLK_ERR_SIZE); G2 in plk_pairing_check's words; a commitment in flight: PLK_ERR_ARG.
 *                Kernels per pass: one lane per opening checks it and writes the count + 3 scalars (the <= 28 differences of the points
 *                inverted by ONE inversion, no count x npoints array in a lane); one lane per (opening, term), count + 3 times as many,
 *                multiplies (g1_mul_dev.h, window table in LDS; a zero scalar or the identity costs nothing); one lane per opening sums its
 *                products with the complete addition (equal terms double, opposite terms cancel) into A, B = -W';
 *                plk_pairing_check_many_dev's kernel decides e(A, Q_0) e(B, Q_1) == 1.  Memory: (count + 3) x 176 B + npoints
 *                (npoints - 1) / 2 x 32 B + 130 B per opening, at most 2^16 openings and 64 MiB per pass (9216 openings at 32 x 8), in
 *                plk_kzg_verify_many_dev's grows-only buffer outside the staging arena.
 *                BREAK-EVEN (one MI355X, profiles/kzg_verify_multi_many.txt): a call costs 89 - 94 ms whatever the batch up to 4096 openings
 *                (the pairing kernel is 87.5 ms of it; plk_kzg_verify_many_dev at the same n on the same box: 89 ms), a
 *                plk_kzg_verify_multi 13 - 15 ms.  Measured at 1 / 256 / 4096 openings: 90 / 89 / 89 ms at count 3, npoints 3 and 92 / 91 / 94 ms
 *                at count 32, npoints 8, against 13 / 210 / 3268 ms and 15 / 234 / 3701 ms for a loop of plk_kzg_verify_multi on 16 host
 *                threads — 256 is the first measured size at which this call wins (the figures cross near 110 and near 100 openings).
 *                The front (checks and scalars) is 0.6 ms and 2.6 ms of the call, all the new kernels 6.4 ms at 4096 x (32, 8).  Below
 *                about a hundred openings, prefer plk_kzg_verify_multi on host threads.
 *   plk_kzg_verify_multi_front_dev.  The front on its own, as plk_verify_front_dev is for proofs: per opening count + 3 Montgomery scalars
 *                c_0 .. c_{count-1}, -sum_i c_i r_i(u), -Z_T(u), u — what multiplies C_0 .. C_{count-1}, G, W, W' — and a state byte
 *                (any alignment): 1 = the opening goes on to the group arithmetic, 2 = malformed, its scalars are zero.  There is no
 *                state 0 in this scheme.  The same refusals and the same order on `stream`; no G2.                                       */
int32_t plk_kzg_verify_multi_many_dev(plk_ctx *ctx, uint32_t count /* 1..32 */, uint32_t npoints /* 1..8 */, const uint32_t *sets /* host, count masks */,
                                      const void *commitments_dev /* n x count plk_g1_affine */, const void *points_dev /* n x npoints plk_fr */,
                                      const void *evals_dev /* n x count x npoints plk_fr */, const void *gamma_dev /* n */, const void *u_dev /* n */,
                                      const void *proofs_dev /* n x 2: W, W' */, uint64_t n, const uint8_t g2[256], void *verdict_dev /* n bytes */, void *stream);
int32_t plk_kzg_verify_multi_front_dev(plk_ctx *ctx, uint32_t count, uint32_t npoints, const uint32_t *sets,
                                       const void *commitments_dev, const void *points_dev, const void *evals_dev, const void *gamma_dev, const void *u_dev,
                                       const void *proofs_dev, uint64_t n, void *scalars_dev /* n x (count + 3) plk_fr, Montgomery */, void *state_dev /* n bytes */,
                                       void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
