// A witness against its R1CS on the GPU: <A_i, w> * <B_i, w> = <C_i, w> for every constraint, exactly, naming the lowest one that fails.
//
// Mirrors (reference file:line):
//   SetupForProver::validate_witness   src/plonk.rs:127-129  ("quickly validate whether a witness is satisfied")
//   CircomCircuit::synthesize          src/circom_circuit.rs:74-133  (what a constraint is; wire 0 = CS::one(), :78,107-113;
//                                      0 * LC = 0 ignored, :122-123)
// The reference only ever checks the gates bellman's transpiler made of these constraints (plk_validate_witness, prover.hip, is that
// call); this file asks the question on the constraints themselves, so neither a setup nor a key nor this library's transpiler is
// involved.  Layout and host half: r1cs_plan.h.
//
// Three kernels per check:
//   k_r1cs_lc_short   one lane per short LC (fewer than R1CS_LONG_LC_TERMS terms): sum coeff * value[wire] -> lc_vals[3m]
//   k_r1cs_lc_long    one wave per long LC: lanes stride over the terms, the 64 partial sums are combined by a tree of
//                     __shfl_down steps (6 steps x 8 limbs; no LDS, so no barrier and the four waves of a block stay independent)
//   k_r1cs_verdict    one lane per constraint: a * b != c -> atomicMin of the constraint index on one 64-bit word (the pattern of
//                     g1_decode_kernel, keyio.hip): the lowest failing constraint whatever the launch geometry
// Arithmetic: the 8 x 32-bit layer of field_dev.h.  Its add, sub and mul take canonical residues and return canonical residues, so
// THE ACCUMULATOR IS REDUCED AFTER EVERY TERM (reduction interval 1) and an LC of any length stays inside the layer's contract; what
// has to hold for that is that every operand is canonical — the table is (built from parsed coefficients), and every witness
// element a term reads is tested (r1cs_canonical) before it is used.  The zero test is Fp::operator== on canonical residues.
// Montgomery scales: coefficient cR times value vR gives cvR, a sum of those times another gives abR, compared with cR-scaled c.
#include "ctx.h"
#include "r1cs_plan.h"
#include <cstring>
#include <memory>

namespace plk {

constexpr int RT = 256;                                    // threads per block (four waves)
constexpr uint64_t R1CS_NONE = ~0ull;                      // a verdict word while nothing has been refused

struct R1csLcArgs {
    const R1csPlanTerm *terms;
    const uint64_t *off;
    const Fr *table;
    const uint32_t *list;                                  // the LC indices this launch owns
    uint32_t count;
    const Fr *witness;
    Fr *lc_vals;
    unsigned long long *bad_wire;                          // lowest wire read by a term whose element is not canonical
};

// x < r, as the subtraction x - r borrowing out of the top limb
__device__ __forceinline__ bool r1cs_canonical(const Fr &x) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)x.l[i] - FrParams::P[i] - br; br = (d >> 32) & 1; }
    return br != 0;
}

// acc + coeff * value[wire].  Wire 0 is the constant 1 whatever witness[0] holds; table[0] = 1 and table[1] = r - 1 are an
// addition and a subtraction.  A value that is not canonical is reported and replaced by zero (the call then ends with PLK_ERR_ARG
// and nobody reads the sum; the layer's contract holds for the lanes that go on).
__device__ __forceinline__ Fr r1cs_term(const Fr &acc, const R1csPlanTerm t, const R1csLcArgs &a) {
    Fr v;
    if (t.wire == 0) v = Fr::one();
    else {
        v = load_fp(a.witness + t.wire);
        if (!r1cs_canonical(v)) { atomicMin(a.bad_wire, (unsigned long long)t.wire); v = Fr::zero(); }
    }
    if (t.coeff == 0) return add(acc, v);
    if (t.coeff == 1) return sub(acc, v);
    return add(acc, mul(load_fp(a.table + t.coeff), v));
}

__global__ void __launch_bounds__(RT) k_r1cs_lc_short(R1csLcArgs a) {
    const uint32_t i = blockIdx.x * RT + threadIdx.x;
    if (i >= a.count) return;
    const uint32_t j = a.list[i];
    const uint64_t lo = a.off[j], hi = a.off[j + 1];
    Fr acc = Fr::zero();
    for (uint64_t k = lo; k < hi; k++) acc = r1cs_term(acc, a.terms[k], a);
    store_fp(a.lc_vals + j, acc);
}

__global__ void __launch_bounds__(RT) k_r1cs_lc_long(R1csLcArgs a) {
    const uint32_t wave = blockIdx.x * (RT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= a.count) return;                           // uniform over the wave
    const uint32_t j = a.list[wave];
    const uint64_t lo = a.off[j], hi = a.off[j + 1];
    Fr acc = Fr::zero();
    for (uint64_t k = lo + lane; k < hi; k += 64) acc = r1cs_term(acc, a.terms[k], a);
    // lane l <- lane l + lane (l + d), d = 32 .. 1: lane 0 ends with the sum of all 64.  A lane whose partner lies beyond the wave
    // gets its own value back and adds it to itself — a canonical residue nobody reads.
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        Fr o;
#pragma unroll
        for (int i = 0; i < 8; i++) o.l[i] = (uint32_t)__shfl_down((int)acc.l[i], (unsigned)d, 64);
        acc = add(acc, o);
    }
    if (lane == 0) store_fp(a.lc_vals + j, acc);
}

__global__ void __launch_bounds__(RT) k_r1cs_verdict(const Fr *lc_vals, uint64_t m, unsigned long long *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * RT + threadIdx.x;
    if (i >= m) return;
    const Fr a = load_fp(lc_vals + 3 * i), b = load_fp(lc_vals + 3 * i + 1), c = load_fp(lc_vals + 3 * i + 2);
    if (mul(a, b) != c) atomicMin(bad, (unsigned long long)i);
}

}  // namespace plk

struct plk_r1cs {
    int device = 0;
    uint64_t m = 0, num_variables = 0, n_terms = 0;
    uint32_t n_short = 0, n_long = 0;
    plk::DevBuf store;                                     // one allocation holding everything below (read-only after upload)
    const plk::R1csPlanTerm *terms = nullptr;
    const uint64_t *off = nullptr;
    const plk::Fr *table = nullptr;
    const uint32_t *short_lcs = nullptr, *long_lcs = nullptr;
};

using namespace plk;

static inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

static int32_t r1cs_upload_impl(plk_ctx *ctx, const plk_circuit *c, plk_r1cs **out) {
    if (!ctx || !c || !out) { set_error("plk_r1cs_upload: bad argument"); return PLK_ERR_ARG; }
    *out = nullptr;
    R1csPlan P;
    std::string err;
    if (!r1cs_plan_build(c->r1cs, &P, &err)) { set_error("plk_r1cs_upload: " + err); return PLK_ERR_FORMAT; }
    PLK_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<plk_r1cs, void (*)(plk_r1cs *)> R(new plk_r1cs(), plk_r1cs_free);
    R->device = ctx->device;
    R->m = P.num_constraints; R->num_variables = P.num_variables; R->n_terms = P.terms.size();
    R->n_short = (uint32_t)P.short_lcs.size(); R->n_long = (uint32_t)P.long_lcs.size();
    const size_t b_terms = pad256(P.terms.size() * sizeof(R1csPlanTerm)), b_off = pad256(P.off.size() * 8), b_tab = pad256(P.table.size() * sizeof(Fr));
    const size_t b_short = pad256(P.short_lcs.size() * 4), b_long = pad256(P.long_lcs.size() * 4);
    PLK_TRY(R->store.reserve(b_terms + b_off + b_tab + b_short + b_long + 256));
    char *p = R->store.as<char>();
    hipStream_t st = ctx->stream;
    auto put = [&](const void *src, size_t bytes, size_t padded) -> const void * {
        char *dst = p;
        p += padded;
        if (bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
        return dst;
    };
    R->table = static_cast<const Fr *>(put(P.table.data(), P.table.size() * sizeof(Fr), b_tab));      // (32-byte records first: alignment)
    R->off = static_cast<const uint64_t *>(put(P.off.data(), P.off.size() * 8, b_off));
    R->terms = static_cast<const R1csPlanTerm *>(put(P.terms.data(), P.terms.size() * sizeof(R1csPlanTerm), b_terms));
    R->short_lcs = static_cast<const uint32_t *>(put(P.short_lcs.data(), P.short_lcs.size() * 4, b_short));
    R->long_lcs = static_cast<const uint32_t *>(put(P.long_lcs.data(), P.long_lcs.size() * 4, b_long));
    if (!R->table || !R->off || !R->terms || !R->short_lcs || !R->long_lcs) PLK_HIP(hipGetLastError());
    PLK_HIP(hipStreamSynchronize(st));                     // the plan's host vectors go away with this frame
    *out = R.release();
    return PLK_OK;
}

// the check proper: `witness` on the device, complete on stream `s` (or written there by work already enqueued)
static int32_t r1cs_check_impl(plk_ctx *ctx, const plk_r1cs *R, const Fr *witness, Fr *lc_vals, unsigned long long *words, hipStream_t s,
                               const char *who, int32_t *valid, uint64_t *bad_out) {
    StageTimer<5> ev;
    ctx->r1cs_ms_valid = false;
    PLK_TRY(ev.start(ctx));
    auto mark = [&](int k) { return ev.mark(k, s); };
    PLK_TRY(mark(0));
    PLK_HIP(hipMemsetAsync(words, 0xff, 16, s));           // words[0]: lowest failing constraint, words[1]: lowest non-canonical wire read
    R1csLcArgs a;
    a.terms = R->terms; a.off = R->off; a.table = R->table; a.witness = witness; a.lc_vals = lc_vals; a.bad_wire = words + 1;
    PLK_TRY(mark(1));
    if (R->n_short) {
        a.list = R->short_lcs; a.count = R->n_short;
        hipLaunchKernelGGL(k_r1cs_lc_short, dim3((R->n_short + RT - 1) / RT), dim3(RT), 0, s, a);
        PLK_HIP(hipGetLastError());
    }
    PLK_TRY(mark(2));
    if (R->n_long) {
        a.list = R->long_lcs; a.count = R->n_long;
        const uint32_t waves_per_block = RT / 64;
        hipLaunchKernelGGL(k_r1cs_lc_long, dim3((R->n_long + waves_per_block - 1) / waves_per_block), dim3(RT), 0, s, a);
        PLK_HIP(hipGetLastError());
    }
    PLK_TRY(mark(3));
    hipLaunchKernelGGL(k_r1cs_verdict, dim3((uint32_t)((R->m + RT - 1) / RT)), dim3(RT), 0, s, (const Fr *)lc_vals, R->m, words);
    PLK_HIP(hipGetLastError());
    PLK_TRY(mark(4));
    unsigned long long got[2] = {R1CS_NONE, R1CS_NONE};
    PLK_HIP(hipMemcpyAsync(got, words, 16, hipMemcpyDeviceToHost, s));
    PLK_HIP(hipStreamSynchronize(s));                      // the verdict is this call's return value
    if (ev.on) {
        for (int k = 0; k < 3; k++) PLK_TRY(ev.elapsed(k + 1, k + 2, &ctx->r1cs_ms[k]));
        PLK_TRY(ev.elapsed(0, 4, &ctx->r1cs_ms[3]));
        ctx->r1cs_ms_valid = true;
    }
    if (got[1] != R1CS_NONE) {
        set_error(std::string(who) + ": wire " + std::to_string(got[1]) + " holds an element that is not a canonical residue (limbs >= r)");
        return PLK_ERR_ARG;
    }
    *valid = got[0] == R1CS_NONE ? 1 : 0;
    if (bad_out) *bad_out = got[0];
    return PLK_OK;
}

static int32_t r1cs_check_entry(plk_ctx *ctx, const plk_r1cs *R, const void *witness, bool on_device, uint64_t n, int32_t *valid, uint64_t *bad_out, void *stream) {
    const char *who = on_device ? "plk_r1cs_check_witness_dev" : "plk_r1cs_check_witness";
    if (valid) *valid = 0;
    if (bad_out) *bad_out = R1CS_NONE;
    if (!ctx || !R || !valid || (!witness && R->num_variables)) { set_error(std::string(who) + ": bad argument"); return PLK_ERR_ARG; }
    if (on_device && ((uintptr_t)witness & 15u)) { set_error(std::string(who) + ": the witness must be 16-byte aligned"); return PLK_ERR_ARG; }
    if (R->device != ctx->device) { set_error(std::string(who) + ": the R1CS was uploaded to another device"); return PLK_ERR_ARG; }
    if (n < R->num_variables) {
        set_error(std::string(who) + ": the witness has " + std::to_string(n) + " elements, the circuit " + std::to_string(R->num_variables) + " variables");
        return PLK_ERR_ARG;
    }
    if (ctx->msm_enq != ctx->msm_fin) { set_error(std::string(who) + ": a commitment is still in flight on this context"); return PLK_ERR_ARG; }
    if (R->m == 0) { *valid = 1; return PLK_OK; }
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t s = on_device && stream ? (hipStream_t)stream : ctx->stream;
    // lc_vals (3m elements), the two verdict words and, for a host witness, its device copy: all in the staging arena
    const size_t b_lc = pad256(3 * R->m * sizeof(Fr)), b_wit = on_device ? 0 : pad256(R->num_variables * sizeof(Fr));
    PLK_TRY(ctx->stage.reserve(b_lc + 256 + b_wit));
    char *base = ctx->stage.as<char>();
    Fr *lc_vals = reinterpret_cast<Fr *>(base);
    unsigned long long *words = reinterpret_cast<unsigned long long *>(base + b_lc);
    const Fr *w = static_cast<const Fr *>(witness);
    if (!on_device) {
        Fr *d_w = reinterpret_cast<Fr *>(base + b_lc + 256);
        PLK_HIP(hipMemcpyAsync(d_w, witness, R->num_variables * sizeof(Fr), hipMemcpyHostToDevice, s));      // pageable: the caller's buffer is never page-locked
        w = d_w;
    }
    return r1cs_check_impl(ctx, R, w, lc_vals, words, s, who, valid, bad_out);
}

extern "C" {

uint32_t plk_r1cs_long_lc_terms(void) { return R1CS_LONG_LC_TERMS; }
uint64_t plk_r1cs_num_constraints(const plk_r1cs *r) { return r ? r->m : 0; }
uint64_t plk_r1cs_num_variables(const plk_r1cs *r) { return r ? r->num_variables : 0; }
void plk_r1cs_free(plk_r1cs *r) { if (r) { r->store.release(); delete r; } }

int32_t plk_r1cs_upload(plk_ctx *ctx, const plk_circuit *c, plk_r1cs **out) {
    return guarded("plk_r1cs_upload", PLK_ERR_HIP, [&] { return r1cs_upload_impl(ctx, c, out); });
}
int32_t plk_r1cs_check_witness(plk_ctx *ctx, const plk_r1cs *r, const plk_fr *witness_host, uint64_t n, int32_t *valid, uint64_t *bad_out) {
    return guarded("plk_r1cs_check_witness", PLK_ERR_HIP, [&] { return r1cs_check_entry(ctx, r, witness_host, false, n, valid, bad_out, nullptr); });
}
int32_t plk_r1cs_check_witness_dev(plk_ctx *ctx, const plk_r1cs *r, const void *witness_dev, uint64_t n, int32_t *valid, uint64_t *bad_out, void *stream) {
    return guarded("plk_r1cs_check_witness_dev", PLK_ERR_HIP, [&] { return r1cs_check_entry(ctx, r, witness_dev, true, n, valid, bad_out, stream); });
}
int32_t plk_r1cs_last_kernel_ms(plk_ctx *ctx, float out_ms[4]) {
    if (!ctx || !out_ms) { set_error("plk_r1cs_last_kernel_ms: bad argument"); return PLK_ERR_ARG; }
    if (!ctx->r1cs_ms_valid) { set_error("plk_r1cs_last_kernel_ms: no timed witness check on this context (plk_set_kernel_timing)"); return PLK_ERR_ARG; }
    for (int k = 0; k < 4; k++) out_ms[k] = ctx->r1cs_ms[k];
    return PLK_OK;
}

}  // extern "C"
