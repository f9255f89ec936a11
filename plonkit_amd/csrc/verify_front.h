// What verify_many.hip (plk_vk_load, plk_verify_many_packed, plk_verify_many_dev, plk_verify_front_dev) shares with the front kernel: the
// key constants it uploads and the two launchers of verify_front.hip.  The code of a lane is verify_front_dev.h, which only verify_front.hip
// (and the host check program) include for the proofs' front: its out-of-line device functions are emitted once there.
// kzg_multi_verify_dev.h takes FRM and fr_inv_call from it, so kzg_multi_verify.hip carries a second copy of them.
#pragma once
#include <hip/hip_runtime.h>
#include "ec_dev.h"

namespace plk {

// what the kernel needs from the key: omega = omega_of(log2(n + 1)) where n + 1 is a power of two in [2, 2^28], zero otherwise
struct FrontVk {
    uint64_t n, num_inputs;
    uint32_t flags, pad[3];
    Fr non_residues[3];
    Fr omega;
};

// vm_front_kernel on `st`: proof i of the pass is blob[off[i] - bias, off[i + 1] - bias), blob_len bytes in all; an offset pair that decreases
// or leaves the blob gives state 2 and nothing of that proof is read.  full = false: 11 points per proof (the arena layout vm_mul_kernel
// reads); full = true: all 25 terms per proof as plk_verify_terms orders them.  Scalars are 25 per proof either way.
int32_t front_launch(G1Affine *pts, Fr *sc, uint8_t *state, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, uint64_t bias, uint32_t count,
                     const FrontVk *vk, const G1Affine *fixed, bool full, hipStream_t st);
// verdict[i] = pairing[i] where state[i] == 1, else what the front end settled: 0 invalid, PLK_VERDICT_MALFORMED.  verdict may be pairing.
int32_t settle_launch(uint8_t *verdict, const uint8_t *pairing, const uint8_t *state, uint32_t count, hipStream_t st);

}  // namespace plk
