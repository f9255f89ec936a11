/* One setup, a stream of witnesses through the C ABI alone (no Python, no torch): the circuit is loaded once, the setup prepared once, and
 * three .wtns files of that circuit — what a proving service receives, one per request — go through plk_prove_wtns.  What a Rust host that
 * keeps one SetupForProver and calls prove() per witness would do (src/plonk.rs:132-159).  Prints "OK 3" when every proof equals, byte for
 * byte, plk_prove on a circuit object that holds the same witness, a witness with an element >= r is refused with its index and the
 * context proves the next good witness afterwards.  Built (-m "not gpu") and run (-m gpu) by tests/test_witness_stream_c.py:
 *   gcc -std=c99 -O2 -I include tests/host/witness_stream.c -L plonkit_amd/lib -lplonkit_amd -Wl,-rpath,$PWD/plonkit_amd/lib */
#include "plonkit_amd.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CK(x) do { int32_t rc_ = (x); if (rc_ != PLK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, plk_last_error()); exit(1); } } while (0)

static uint8_t *export_bytes(const plk_circuit *c, int32_t what, uint64_t *len) {
    CK(plk_circuit_export(c, what, 0, 0, len));
    uint8_t *b = (uint8_t *)malloc(*len);
    if (!b) { fprintf(stderr, "out of memory\n"); exit(1); }
    CK(plk_circuit_export(c, what, b, *len, len));
    return b;
}

int main(int argc, char **argv) {
    const unsigned log_n = argc > 1 ? (unsigned)atoi(argv[1]) : 12;
    const uint64_t n = 1ull << log_n;
    plk_ctx *ctx = 0;
    CK(plk_create(0, &ctx));
    CK(plk_srs_generate(ctx, n, 0, 42));
    static uint8_t want[3][1 << 16], got[1 << 16];
    uint64_t want_len[3], wlen[3], len = 0, bad = 0;
    uint8_t *wtns[3];
    plk_setup *s = 0;
    for (int k = 0; k < 3; k++) {                                  /* the same R1CS with three witnesses: the bytes a client would send, */
        plk_circuit *c = 0;                                        /* and the proof plk_prove makes of the circuit object                */
        CK(plk_circuit_synthetic_ex(n - 2, 7, (uint64_t)k + 1, 0, &c));
        if (k == 0) CK(plk_setup_prepare(ctx, c, &s));
        wtns[k] = export_bytes(c, 1, &wlen[k]);
        CK(plk_prove(ctx, s, c, want[k], sizeof want[k], &want_len[k]));
        plk_circuit_free(c);                                       /* only the setup and the witness bytes live on */
    }
    if (want_len[0] == want_len[1] && memcmp(want[0], want[1], want_len[0]) == 0) { fprintf(stderr, "reference proofs do not differ\n"); return 1; }
    for (int k = 0; k < 3; k++) {
        CK(plk_prove_wtns(ctx, s, wtns[k], wlen[k], got, sizeof got, &len, &bad));
        if (len != want_len[k] || memcmp(got, want[k], len) != 0 || bad != UINT64_MAX) { fprintf(stderr, "proof %d differs from plk_prove's\n", k); return 1; }
    }
    memset(wtns[1] + 76 + 32 * 5, 0xff, 32);                       /* element 5 >= r */
    if (plk_prove_wtns(ctx, s, wtns[1], wlen[1], got, sizeof got, &len, &bad) != PLK_ERR_FORMAT || bad != 5 || len != 0) {
        fprintf(stderr, "an element that is not in the field was not refused: %s\n", plk_last_error()); return 1; }
    CK(plk_prove_wtns(ctx, s, wtns[2], wlen[2], got, sizeof got, &len, &bad));
    if (len != want_len[2] || memcmp(got, want[2], len) != 0) { fprintf(stderr, "the proof after a refusal differs\n"); return 1; }
    for (int k = 0; k < 3; k++) free(wtns[k]);
    plk_setup_free(s);
    plk_destroy(ctx);
    printf("OK 3\n");
    return 0;
}
