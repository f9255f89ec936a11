// Device side of the assembled-input path (plk_setup_from_polynomials / plk_prove_assembled*): the setup polynomials and the four
// wire columns arrive as vectors that bellman's own synthesis produced (SetupPolynomials, src/plonk.rs:50-55,104; the prover assembly
// behind prove_by_steps, src/plonk.rs:152-159) instead of this library's transpiler.  What the gate structure gave the circuit path for
// free has to be checked here: every element is a canonical residue, the columns satisfy every gate, and (prover.hip, round 2) the copy
// constraints of the caller's sigma hold.
#include "ctx.h"
#include "poly.h"

namespace plk {

constexpr int PT = 256;

// x < r, as the subtraction x - r borrowing out of the top limb
__device__ __forceinline__ bool fr_canonical(const Fr &x) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)x.l[i] - FrParams::P[i] - br; br = (d >> 32) & 1; }
    return br != 0;
}

// bit v of *flag <- some element of vector v (blockIdx.y) is not canonical
struct CanonBatch { const Fr *v[CANON_MAX]; };
__global__ void __launch_bounds__(PT) k_check_canonical(CanonBatch a, uint32_t len, uint32_t *flag) {
    const uint32_t i = blockIdx.x * PT + threadIdx.x, v = blockIdx.y;
    if (i < len && !fr_canonical(load_fp(a.v[v] + i))) atomicOr(flag, 1u << v);
}

// One pass over the four caller columns (row r of a, b, c, d per lane): canonical check (flag[0], bit j = column j), zero padding from
// `rows` to n, both copies the prover needs (w_vals for the grand product, w_coef for the round-1 iNTT in place), and the width-4 gate
// equation of k_check_gates (poly.hip) on the column values, public-input term included: flag[1] = max over failing rows of n - r, i.e.
// the lowest failing row is n - flag[1] (0: every gate holds).  d_next of the last row is zero, as in k_check_gates.
__global__ void __launch_bounds__(PT) k_ingest_columns(IngestArgs a) {
    const uint32_t r = blockIdx.x * PT + threadIdx.x;
    if (r >= a.n) return;
    const bool live = r < a.rows;
    Fr w[4];
    uint32_t bad = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        w[j] = live ? load_fp(a.src[j] + r) : Fr::zero();
        if (!fr_canonical(w[j])) bad |= 1u << j;
        store_fp(a.vals[j] + r, w[j]);
        store_fp(a.coef[j] + r, w[j]);
    }
    Fr acc = load_fp(a.q[5] + r);
#pragma unroll
    for (int j = 0; j < 4; j++) acc = add(acc, mul(load_fp(a.q[j] + r), w[j]));
    acc = add(acc, mul(load_fp(a.q[4] + r), mul(w[0], w[1])));
    const Fr qn = load_fp(a.q[6] + r);
    if (!qn.is_zero()) {
        const Fr dn = r + 1 < a.rows ? load_fp(a.src[3] + r + 1) : Fr::zero();
        acc = add(acc, mul(qn, dn));
    }
    if (r < a.num_inputs) acc = add(acc, w[0]);
    if (bad) atomicOr(a.flag, bad);
    if (!acc.is_zero()) atomicMax(a.flag + 1, a.n - r);
}

int32_t check_canonical(const Fr *const *v, uint32_t count, uint64_t len, uint32_t *flag, hipStream_t s) {
    if (count > CANON_MAX || len > 0xffffffffull) { set_error("check_canonical: bad argument"); return PLK_ERR_ARG; }
    if (!count || !len) return PLK_OK;
    CanonBatch a;
    for (uint32_t k = 0; k < count; k++) a.v[k] = v[k];
    hipLaunchKernelGGL(k_check_canonical, dim3((uint32_t)((len + PT - 1) / PT), count), dim3(PT), 0, s, a, (uint32_t)len, flag);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

int32_t ingest_columns(const IngestArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_ingest_columns, dim3((a.n + PT - 1) / PT), dim3(PT), 0, s, a);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

}  // namespace plk
