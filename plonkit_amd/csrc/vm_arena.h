// The working memory of one pass of the batch verifiers (verify_many.hip): where each array lies, as pure functions of integers.
// Host code only: no HIP include, so a stand-alone program can check it (tests/host/vm_arena_check.cpp).
// NO COUNTERPART IN THE REFERENCE, whose plonk::verify (src/plonk.rs:189-210) takes one proof.
//
// m proofs, every part 16-byte aligned, in this order:
//   pts     m x 11 affine points     the proof's commitments
//   sc      m x 25 Fr                the flattened scalars
//   prod    m x 25 XYZZ (29-bit)     the products
//   sum     m x 2 XYZZ               the two sides of the pairing equation
//   aff     m x 2 affine points      the same, normalised
//   v       m bytes                  the pairing verdicts
//   state   m bytes                  what the front kernel settled
// and behind them, each only where the call has it:
//   keys    m x u32                  the key index per proof (a key set, blocking calls)
//   off     (m + 1) x u64            the pass's offsets into the raw bytes (plk_verify_*_packed)
//   blob    blob_bytes               the raw bytes of the pass (plk_verify_*_packed)
// The host front end has no use for `state` and reserves it all the same: at most 64 KiB per 2^16 proofs, for one layout instead of two.
#pragma once
#include <cstddef>
#include <cstdint>

namespace plk {

constexpr size_t VM_ARENA_PTS = 11, VM_ARENA_TERMS = 25;                  // points a proof brings: VM_PROOF_PTS and VERIFY_TERMS of verify_many.hip
constexpr size_t VM_AFFINE_BYTES = 64, VM_FR_BYTES = 32, VM_XYZZW_BYTES = 144, VM_XYZZ_BYTES = 128;

inline size_t vm_pad16(size_t b) { return (b + 15) & ~(size_t)15; }

struct VmLayout {
    size_t pts, sc, prod, sum, aff, v, state, keys, off, blob, bytes;   // byte offsets of the parts, and the size of the whole
};

// raw: the pass takes its proofs as raw bytes uploaded by the call, blob_bytes of them (ignored otherwise)
inline VmLayout vm_layout(size_t m, bool keys, bool raw, size_t blob_bytes) {
    VmLayout L;
    L.pts = 0;
    L.sc = L.pts + m * VM_ARENA_PTS * VM_AFFINE_BYTES;
    L.prod = L.sc + m * VM_ARENA_TERMS * VM_FR_BYTES;
    L.sum = L.prod + m * VM_ARENA_TERMS * VM_XYZZW_BYTES;
    L.aff = L.sum + m * 2 * VM_XYZZ_BYTES;
    L.v = L.aff + m * 2 * VM_AFFINE_BYTES;
    L.state = L.v + vm_pad16(m);
    L.keys = L.state + vm_pad16(m);
    L.off = L.keys + (keys ? vm_pad16(m * sizeof(uint32_t)) : 0);
    L.blob = L.off + (raw ? vm_pad16((m + 1) * sizeof(uint64_t)) : 0);
    L.bytes = L.blob + (raw ? vm_pad16(blob_bytes) : 0);
    return L;
}

}  // namespace plk
