// The device side of a key set (plk_vkset): the view of the image vkset_plan.h lays out, and the ONE function through which a lane goes
// from a key index to what it needs of that key.  vkset_lookup is __host__ __device__: tests/host/verify_mixed_check.hip runs it on an
// image built in host memory.  Used by vm_front_mixed_kernel (verify_front.hip), vm_mul_mixed_kernel and vm_pairing_mixed_kernel
// (verify_many.hip).  NO COUNTERPART IN THE REFERENCE.
#pragma once
#include "verify_front.h"
#include "fq12_dev.h"
#include "vkset_plan.h"

namespace plk {

static_assert(sizeof(FrontVk) == VKSET_FRONT_BYTES && sizeof(G1Affine) * 12 == VKSET_FIXED_BYTES, "vkset_plan.h lays the image out without these types");

struct VksetView {
    const FrontVk *front;          // n_keys
    const G1Affine *fixed;         // n_keys x 12
    const uint32_t *table_of;      // n_keys
    const char *tables;            // n_tables x table_stride: [PairingHead | lines]
    uint64_t table_stride;
    uint32_t n_keys, n_tables;
};

struct VksetKey {
    const FrontVk *front;
    const G1Affine *fixed;         // 12 points
    const PairingHead *head;
    const Fq *lines;
};

inline VksetView vkset_view(const void *image, const VksetLayout &L) {
    const char *b = reinterpret_cast<const char *>(image);
    VksetView v;
    v.front = reinterpret_cast<const FrontVk *>(b + L.front_off);
    v.fixed = reinterpret_cast<const G1Affine *>(b + L.fixed_off);
    v.table_of = reinterpret_cast<const uint32_t *>(b + L.index_off);
    v.tables = b + L.tables_off;
    v.table_stride = L.table_stride;
    v.n_keys = L.n_keys; v.n_tables = L.n_tables;
    return v;
}

// false: `key` is out of range (or the image names a table it does not hold) and nothing of the image past table_of[key] is touched
PLK_HD bool vkset_lookup(const VksetView &v, uint32_t key, VksetKey *out) {
    if (key >= v.n_keys) return false;
    const uint32_t t = v.table_of[key];
    if (t >= v.n_tables) return false;
    const char *tab = v.tables + (uint64_t)t * v.table_stride;
    out->front = v.front + key;
    out->fixed = v.fixed + (uint64_t)key * 12;
    out->head = reinterpret_cast<const PairingHead *>(tab);
    out->lines = reinterpret_cast<const Fq *>(tab + sizeof(PairingHead));
    return true;
}

// vm_front_mixed_kernel on `st` (verify_front.hip): front_launch with full = false, proof i under key key_of[i]; a key index out of range gives
// state 2 before off[i] is read
int32_t front_mixed_launch(G1Affine *pts, Fr *sc, uint8_t *state, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, uint64_t bias, uint32_t count,
                           const VksetView &set, const uint32_t *key_of, hipStream_t st);

}  // namespace plk
