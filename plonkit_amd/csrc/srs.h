// What srs.hip shares with the key update (srs_update.hip): the chunk size of a pass through an XYZZ scratch and the kernel
// that brings such a scratch to affine.
#pragma once
#include "ctx.h"
#include "ec_dev.h"

namespace plk {

constexpr uint64_t SRS_CHUNK = 1ull << 22;       // points per pass through the XYZZ scratch (512 MiB)

// out[i] = in[i] in affine coordinates, i < n (external form on both sides; infinity = all zero), one inversion per eight points
int32_t srs_to_affine(G1Affine *out, const G1Xyzz *in, uint64_t n, hipStream_t s);

}  // namespace plk
