// Stand-alone check of plonkit_amd/csrc/vm_arena.h, the layout of the batch verifiers' working memory.  Built with AddressSanitizer and UBSan
// and run directly by tests/test_vm_arena_host.py.  For m in {1, 15, 16, 17, 65535, 65536}, every combination of the optional parts and raw
// byte counts 0, 1, 15 and 16: the parts lie in the documented order, each starts 16-byte aligned, no two overlap, the last ends within
// bytes, and bytes does not decrease as m grows.  The seven fixed parts lie where the arena of the packed calls had them before the layout
// moved into the header; that formula is written out once below, in bytes per proof.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../plonkit_amd/csrc/vm_arena.h"

using namespace plk;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { printf("vm_arena_check: line %d: %s (m = %zu, keys %d, raw %d, %zu bytes)\n", __LINE__, #cond, m, (int)keys, (int)raw, blob); return 1; } \
    } while (0)

struct Part { const char *name; size_t at, len; };

int main() {
    const size_t ms[] = {1, 15, 16, 17, 65535, 65536}, blobs[] = {0, 1, 15, 16};
    int shapes = 0;
    for (int keys = 0; keys < 2; keys++)
        for (int raw = 0; raw < 2; raw++)
            for (size_t blob : blobs) {
                if (!raw && blob) continue;
                size_t last_bytes = 0;
                for (size_t m : ms) {
                    const VmLayout L = vm_layout(m, keys != 0, raw != 0, blob);
                    // what each part holds, from the header's table
                    const Part parts[] = {{"pts", L.pts, m * 11 * 64}, {"sc", L.sc, m * 25 * 32}, {"prod", L.prod, m * 25 * 144}, {"sum", L.sum, m * 2 * 128},
                                          {"aff", L.aff, m * 2 * 64}, {"v", L.v, m}, {"state", L.state, m}, {"keys", L.keys, keys ? m * 4 : 0},
                                          {"off", L.off, raw ? (m + 1) * 8 : 0}, {"blob", L.blob, raw ? blob : 0}};
                    const size_t n = sizeof parts / sizeof parts[0];
                    CHECK(parts[0].at == 0);
                    for (size_t k = 0; k < n; k++) {
                        CHECK(parts[k].at % 16 == 0);
                        CHECK(parts[k].at + parts[k].len <= L.bytes);
                        if (k + 1 < n) CHECK(parts[k].at + parts[k].len <= parts[k + 1].at);      // in order, and so disjoint
                    }
                    // the arena of the packed calls as it was carved by hand: 704 + 800 + 3600 + 256 + 128 bytes per proof, then two padded byte arrays
                    const size_t pad = (m + 15) / 16 * 16;
                    CHECK(L.sc == m * 704 && L.prod == m * 1504 && L.sum == m * 5104 && L.aff == m * 5360 && L.v == m * 5488 && L.state == m * 5488 + pad);
                    CHECK(L.keys == m * 5488 + 2 * pad);
                    // an absent part takes no room, a present one is not padded by more than 15 bytes
                    CHECK(L.bytes - L.keys < (keys ? m * 4 : 0) + (raw ? (m + 1) * 8 + blob : 0) + 48);
                    CHECK(L.bytes >= last_bytes);
                    last_bytes = L.bytes;
                    shapes++;
                }
            }
    // the device form reserves for a full chunk once and carves shorter passes out of it
    for (size_t m : ms) {
        const size_t keys = 0, raw = 0, blob = 0;
        CHECK(vm_layout(m, false, false, 0).bytes <= vm_layout(65536, false, false, 0).bytes);
    }
    printf("vm_arena_check: ok (%d shapes)\n", shapes);
    return 0;
}
