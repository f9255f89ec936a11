// vm_front_kernel: the verifier's front end on the device, one proof per lane — proof bytes in, the proof's 11 points, the 25 flattened
// scalars and a state byte out, in the layout vm_mul_kernel (verify_many.hip) reads.  NO COUNTERPART IN THE REFERENCE.  The code of a lane is
// verify_front_dev.h, which tests/host/verify_front_check.hip runs on the CPU against verify.cpp.
//
// Bounds: lane i reads off[i] and off[i + 1] (the table has count + 1 entries), and of the blob only [off[i] - bias, off[i + 1] - bias) after
// that pair has been checked to be ordered and inside [bias, bias + blob_len]; inside a proof front_parse compares before every read.  It
// writes pts[i * stride .. + stride), sc[i * 25 .. + 25) and state[i] (an ordinary byte store), nothing else.
// One wave per workgroup, as the pairing kernel: a small batch still spreads over the CUs.  A lane's chain is ~80 permutations and
// num_inputs + 1 inversions; lanes that settle early idle until their wave ends.
// vm_front_mixed_kernel is the same lane code for a key set (plk_verify_mixed_packed, plk_verify_mixed_dev): the FrontVk of lane i is that of
// key key_of[i], through vkset_lookup (vkset_dev.h).
#include "ctx.h"
#include "verify_front_dev.h"
#include "verify_many.h"
#include "vkset_dev.h"

namespace plk {

constexpr uint32_t VF_THREADS = 64;

__global__ void __launch_bounds__(VF_THREADS) vm_front_kernel(G1Affine *pts, Fr *sc, uint8_t *state, const uint8_t *blob, uint64_t blob_len, const uint64_t *off,
                                                              uint64_t bias, uint32_t count, const FrontVk *vkp, const G1Affine *fixed, uint32_t full) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t stride = full ? (uint32_t)VERIFY_TERMS : (uint32_t)FRONT_PTS, first = full ? 11u : 0u;
    G1Affine *p = pts + (size_t)i * stride;
    Fr *s = sc + (size_t)i * VERIFY_TERMS;
    const FrontVk vk = *vkp;
    const uint64_t lo = off[i], hi = off[i + 1];
    uint32_t st = FRONT_MALFORMED;
    if (lo >= bias && hi >= lo && hi - bias <= blob_len) st = flatten_front(vk, blob + (lo - bias), blob + (hi - bias), p + first, s);
    if (st == FRONT_GOES_ON) {
        if (full) {                                                   // terms 0..10 and 22 are the key's, 23 and 24 repeat W_z and W_zw
            for (uint32_t k = 0; k < 11; k++) { const G1Affine f = load_affine(fixed + k); store_fp(&p[k].x, f.x); store_fp(&p[k].y, f.y); }
            const G1Affine g = load_affine(fixed + 11), wz = load_affine(p + 20), wzw = load_affine(p + 21);
            store_fp(&p[22].x, g.x); store_fp(&p[22].y, g.y);
            store_fp(&p[23].x, wz.x); store_fp(&p[23].y, wz.y);
            store_fp(&p[24].x, wzw.x); store_fp(&p[24].y, wzw.y);
        }
    } else {
        const Fq zq = Fq::zero(); const Fr zr = Fr::zero();
        for (uint32_t k = 0; k < stride; k++) { store_fp(&p[k].x, zq); store_fp(&p[k].y, zq); }
        for (uint32_t k = 0; k < (uint32_t)VERIFY_TERMS; k++) store_fp(&s[k], zr);
    }
    state[i] = (uint8_t)st;
}

// vm_front_kernel for a key set (plk_verify_mixed*): lane i takes its FrontVk through key_of[i].  The arena layout only (11 points per proof:
// vm_mul_mixed_kernel fetches the key's points itself).  A key index out of range gives state 2 before off[i] is read.
__global__ void __launch_bounds__(VF_THREADS) vm_front_mixed_kernel(G1Affine *pts, Fr *sc, uint8_t *state, const uint8_t *blob, uint64_t blob_len, const uint64_t *off,
                                                                    uint64_t bias, uint32_t count, VksetView set, const uint32_t *key_of) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    G1Affine *p = pts + (size_t)i * FRONT_PTS;
    Fr *s = sc + (size_t)i * VERIFY_TERMS;
    uint32_t st = FRONT_MALFORMED;
    VksetKey key;
    if (vkset_lookup(set, key_of[i], &key)) {
        const FrontVk vk = *key.front;
        const uint64_t lo = off[i], hi = off[i + 1];
        if (lo >= bias && hi >= lo && hi - bias <= blob_len) st = flatten_front(vk, blob + (lo - bias), blob + (hi - bias), p, s);
    }
    if (st != FRONT_GOES_ON) {
        const Fq zq = Fq::zero(); const Fr zr = Fr::zero();
        for (uint32_t k = 0; k < (uint32_t)FRONT_PTS; k++) { store_fp(&p[k].x, zq); store_fp(&p[k].y, zq); }
        for (uint32_t k = 0; k < (uint32_t)VERIFY_TERMS; k++) store_fp(&s[k], zr);
    }
    state[i] = (uint8_t)st;
}

__global__ void __launch_bounds__(256) vm_settle_kernel(uint8_t *verdict, const uint8_t *pairing, const uint8_t *state, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint8_t st = state[i];
    verdict[i] = st == FRONT_GOES_ON ? pairing[i] : st == FRONT_MALFORMED ? (uint8_t)PLK_VERDICT_MALFORMED : (uint8_t)0;
}

int32_t front_launch(G1Affine *pts, Fr *sc, uint8_t *state, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, uint64_t bias, uint32_t count,
                     const FrontVk *vk, const G1Affine *fixed, bool full, hipStream_t st) {
    hipLaunchKernelGGL(vm_front_kernel, dim3((count + VF_THREADS - 1) / VF_THREADS), dim3(VF_THREADS), 0, st, pts, sc, state, blob, blob_len, off, bias, count, vk, fixed,
                       full ? 1u : 0u);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

int32_t front_mixed_launch(G1Affine *pts, Fr *sc, uint8_t *state, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, uint64_t bias, uint32_t count,
                           const VksetView &set, const uint32_t *key_of, hipStream_t st) {
    hipLaunchKernelGGL(vm_front_mixed_kernel, dim3((count + VF_THREADS - 1) / VF_THREADS), dim3(VF_THREADS), 0, st, pts, sc, state, blob, blob_len, off, bias, count, set,
                       key_of);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

int32_t settle_launch(uint8_t *verdict, const uint8_t *pairing, const uint8_t *state, uint32_t count, hipStream_t st) {
    hipLaunchKernelGGL(vm_settle_kernel, dim3((count + 255) / 256), dim3(256), 0, st, verdict, pairing, state, count);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

}  // namespace plk
