/* The library's own rolling Keccak behind a plk_transcript_ops table, in C, so that tools/transcript_ops_ab.py can time what the
 * indirection through the callbacks costs against the built-in transcript (about 30 indirect calls per proof) without a Python frame in
 * the way.  gcc -O2 -shared -fPIC -I include tools/transcript_keccak_shim.c -o tools/tmp_transcript_keccak_shim.so -L plonkit_amd/lib -lplonkit_amd */
#include "plonkit_amd.h"
#include <stdlib.h>

static int32_t kk_begin(void *user, void **state) {
    plk_transcript *t = (plk_transcript *)malloc(sizeof *t);
    (void)user;
    if (!t) return 1;
    plk_transcript_init(t);
    *state = t;
    return 0;
}
static int32_t kk_fr(void *state, const plk_fr *v) { plk_transcript_absorb_fr((plk_transcript *)state, v); return 0; }
static int32_t kk_g1(void *state, const plk_g1_affine *p) { plk_transcript_absorb_g1((plk_transcript *)state, p); return 0; }
static int32_t kk_challenge(void *state, plk_fr *out) { plk_transcript_challenge((plk_transcript *)state, out); return 0; }
static void kk_end(void *user, void *state) { (void)user; free(state); }

__attribute__((visibility("default"))) void shim_keccak_ops(plk_transcript_ops *out) {
    out->user = 0; out->begin = kk_begin; out->absorb_fr = kk_fr; out->absorb_g1 = kk_g1; out->challenge = kk_challenge; out->end = kk_end; out->flags = 0;
}
