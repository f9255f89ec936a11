// The host side of a key set (plk_vkset, verify_many.hip): which keys share a line table, where everything lies in the set's one device
// allocation, whether a caller's key-index array is usable, and the compaction of the (proof, key) pairs the host front end lets through.
// Host code only: no HIP include, so a stand-alone program can check it (tests/host/verify_mixed_check.hip).
// NO COUNTERPART IN THE REFERENCE, whose plonk::verify (src/plonk.rs:189-210) takes one key and one proof.
//
// Image, every part 16-byte aligned, n keys and T distinct G2 pairs:
//   front     n x VKSET_FRONT_BYTES   the FrontVk of key k (sizes, flags, non-residues, omega)
//   fixed     n x VKSET_FIXED_BYTES   its 11 commitments and the generator (terms 0..10 and 22)
//   table_of  n x u32                 the index of its line table, < T
//   tables    T x table_stride        [PairingHead | lines] of each distinct G2 pair, in order of first appearance among the keys
// Two keys share a table exactly when their 256 G2 bytes are equal.  The line count is the same for every pair, so one stride serves all.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace plk {

constexpr uint32_t VKSET_MAX_KEYS = 1024;                           // PLK_VKSET_MAX_KEYS
constexpr size_t VKSET_FRONT_BYTES = 160, VKSET_FIXED_BYTES = 12 * 64, VKSET_G2_BYTES = 256;

// table_of[k] for the n keys whose G2 bytes lie back to back in g2, first_key[t] = the first key of table t; returns T
inline uint32_t vkset_dedup(const uint8_t *g2, uint32_t n, std::vector<uint32_t> *table_of, std::vector<uint32_t> *first_key) {
    table_of->assign(n, 0);
    first_key->clear();
    for (uint32_t k = 0; k < n; k++) {
        uint32_t t = 0;
        while (t < first_key->size() && memcmp(g2 + (size_t)(*first_key)[t] * VKSET_G2_BYTES, g2 + (size_t)k * VKSET_G2_BYTES, VKSET_G2_BYTES) != 0) t++;
        if (t == first_key->size()) first_key->push_back(k);
        (*table_of)[k] = t;
    }
    return (uint32_t)first_key->size();
}

struct VksetLayout {
    uint32_t n_keys = 0, n_tables = 0;
    size_t front_off = 0, fixed_off = 0, index_off = 0, tables_off = 0, table_stride = 0, bytes = 0;
};

inline size_t vkset_pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// table_bytes: sizeof(PairingHead) + lines x 8 Fq of one G2 pair
inline VksetLayout vkset_layout(uint32_t n_keys, uint32_t n_tables, size_t table_bytes) {
    VksetLayout L;
    L.n_keys = n_keys; L.n_tables = n_tables;
    L.front_off = 0;
    L.fixed_off = L.front_off + (size_t)n_keys * VKSET_FRONT_BYTES;
    L.index_off = L.fixed_off + (size_t)n_keys * VKSET_FIXED_BYTES;
    L.tables_off = L.index_off + vkset_pad16((size_t)n_keys * sizeof(uint32_t));
    L.table_stride = vkset_pad16(table_bytes);
    L.bytes = L.tables_off + (size_t)n_tables * L.table_stride;
    return L;
}

// true when every key_of[i] < n_keys; else *first_bad = the lowest i that is not
inline bool vkset_indices_ok(const uint32_t *key_of, uint64_t count, uint32_t n_keys, uint64_t *first_bad) {
    for (uint64_t i = 0; i < count; i++) if (key_of[i] >= n_keys) { *first_bad = i; return false; }
    return true;
}

// the proofs of a pass that go on to the device (mark[i] == 0xff), in index order, each with the key it was checked under
inline void vkset_compact(const uint8_t *mark, const uint32_t *key_of, uint64_t cnt, std::vector<uint64_t> *live, std::vector<uint32_t> *live_key) {
    live->clear(); live_key->clear();
    for (uint64_t i = 0; i < cnt; i++) if (mark[i] == 0xff) { live->push_back(i); live_key->push_back(key_of[i]); }
}

}  // namespace plk
