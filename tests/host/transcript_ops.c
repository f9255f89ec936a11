/* A transcript of the caller's through the C ABI alone (no Python): what a Rust host that owns a `T: Transcript<Fr>` this library does not
 * have would do for the "rescue" arms of src/plonk.rs:160-169,198-204 — hand it over as a plk_transcript_ops table.  The transcript here is
 * a stand-in written over the exported plk_keccak256: ONE 32-byte state, state' = keccak(tag | state | the element's in-memory bytes) with
 * the tags 0xA1 (Fr) and 0xA2 (G1), and a challenge keccak(0xA3 | state) that also becomes part of the next state and is REDUCED below r
 * (not masked), read as the challenge's in-memory words.  Every begin allocates its state and every end frees it, so a missing or doubled
 * end is a leak or a double free under the sanitizers; the two counters must agree at the end.
 *   transcript_ops host vk.bin proof.bin   no GPU: Keccak routed through the callbacks (they call plk_transcript_*) accepts the golden
 *                                          pair, the stand-in refuses it, a failing callback and a challenge >= r are errors, and the
 *                                          truncated proof never reaches begin.  Also built with -fsanitize=address,undefined against
 *                                          the host sources (tests/host/sanitize_transcript_ops.cpp; -DTRANSCRIPT_OPS_HOST_ONLY).
 *   transcript_ops gpu                     plk_prove_witness under the stand-in (PLK_TRANSCRIPT_CONCURRENT unset), then a batch of those
 *                                          proofs with a Keccak proof, a tampered and a truncated one through plk_verify_many_with with
 *                                          the flag SET; every verdict must be plk_verify_with's.
 * Prints "OK <checks>".  Built (-m "not gpu") and run (host: -m "not gpu", gpu: -m gpu) by tests/test_transcript_ops_c.py. */
#include "plonkit_amd.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CK(x) do { int32_t rc_ = (x); if (rc_ != PLK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, plk_last_error()); exit(1); } } while (0)
#define WANT(cond, what) do { if (!(cond)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, what, plk_last_error()); exit(1); } checks++; } while (0)

static int checks = 0;
static const uint64_t R_LIMBS[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

/* ---- the stand-in transcript */
typedef struct { int begins, ends, calls, fail_at; int big_challenge; } alt_user;   /* fail_at: 1-based call after begin that returns 5 */
typedef struct { uint8_t state[32]; alt_user *u; } alt_state;

static int alt_count(alt_state *s) { return __sync_add_and_fetch(&s->u->calls, 1) == s->u->fail_at; }
static void alt_mix(alt_state *s, uint8_t tag, const void *data, size_t len) {
    uint8_t buf[1 + 32 + 64];
    buf[0] = tag; memcpy(buf + 1, s->state, 32); memcpy(buf + 33, data, len);
    plk_keccak256(buf, 33 + len, s->state);
}
static int32_t alt_begin(void *user, void **state) {
    alt_state *s = (alt_state *)malloc(sizeof *s);
    if (!s) return 1;
    memset(s->state, 0x5a, 32);
    s->u = (alt_user *)user;
    __sync_add_and_fetch(&s->u->begins, 1);
    *state = s;
    return 0;
}
static int32_t alt_fr(void *state, const plk_fr *v) { alt_state *s = (alt_state *)state; if (alt_count(s)) return 5; alt_mix(s, 0xA1, v, 32); return 0; }
static int32_t alt_g1(void *state, const plk_g1_affine *p) { alt_state *s = (alt_state *)state; if (alt_count(s)) return 5; alt_mix(s, 0xA2, p, 64); return 0; }
static int geq_r(const uint64_t l[4]) {
    for (int i = 3; i >= 0; i--) { if (l[i] > R_LIMBS[i]) return 1; if (l[i] < R_LIMBS[i]) return 0; }
    return 1;
}
static int32_t alt_challenge(void *state, plk_fr *out) {
    alt_state *s = (alt_state *)state;
    uint8_t d[32];
    if (alt_count(s)) return 5;
    { uint8_t buf[33]; buf[0] = 0xA3; memcpy(buf + 1, s->state, 32); plk_keccak256(buf, 33, d); }
    alt_mix(s, 0xA4, d, 32);
    for (int i = 0; i < 4; i++) { uint64_t w = 0; for (int b = 7; b >= 0; b--) w = (w << 8) | d[8 * i + b]; out->l[i] = w; }
    if (s->u->big_challenge) { memcpy(out->l, R_LIMBS, 32); return 0; }
    while (geq_r(out->l)) {                                          /* 2^256 < 6 r: at most five subtractions */
        uint64_t borrow = 0;
        for (int i = 0; i < 4; i++) {
            const uint64_t a = out->l[i], b = R_LIMBS[i], t = a - b - borrow;
            borrow = (a < b) || (a == b && borrow);
            out->l[i] = t;
        }
    }
    return 0;
}
static void alt_end(void *user, void *state) { __sync_add_and_fetch(&((alt_user *)user)->ends, 1); free(state); }
static plk_transcript_ops alt_ops(alt_user *u, uint32_t flags) {
    plk_transcript_ops o;
    memset(&o, 0, sizeof o);
    o.user = u; o.begin = alt_begin; o.absorb_fr = alt_fr; o.absorb_g1 = alt_g1; o.challenge = alt_challenge; o.end = alt_end; o.flags = flags;
    return o;
}

/* ---- the library's own Keccak transcript routed through the callbacks */
static int32_t kk_begin(void *user, void **state) {
    plk_transcript *t = (plk_transcript *)malloc(sizeof *t);
    if (!t) return 1;
    plk_transcript_init(t); *state = t; ++*(int *)user;
    return 0;
}
static int32_t kk_fr(void *state, const plk_fr *v) { plk_transcript_absorb_fr((plk_transcript *)state, v); return 0; }
static int32_t kk_g1(void *state, const plk_g1_affine *p) { plk_transcript_absorb_g1((plk_transcript *)state, p); return 0; }
static int32_t kk_challenge(void *state, plk_fr *out) { plk_transcript_challenge((plk_transcript *)state, out); return 0; }
static void kk_end(void *user, void *state) { --*(int *)user; free(state); }

static uint8_t *slurp(const char *path, uint64_t *len) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END); *len = (uint64_t)ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t *b = (uint8_t *)malloc(*len + 1);
    if (!b || fread(b, 1, *len, f) != *len) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return b;
}

static int host_half(const char *vk_path, const char *proof_path) {
    uint64_t vk_len, proof_len;
    uint8_t *vk = slurp(vk_path, &vk_len), *proof = slurp(proof_path, &proof_len);
    int32_t valid = -1, early = -1;
    int open_states = 0;
    plk_transcript_ops kk;
    memset(&kk, 0, sizeof kk);
    kk.user = &open_states; kk.begin = kk_begin; kk.absorb_fr = kk_fr; kk.absorb_g1 = kk_g1; kk.challenge = kk_challenge; kk.end = kk_end;
    CK(plk_verify_with(vk, vk_len, proof, proof_len, 0, &kk, &valid));
    WANT(valid == 1 && open_states == 0, "Keccak through the callbacks must accept the golden proof");
    {   /* the flattened form is plk_verify_terms's, bit for bit */
        static plk_g1_affine p0[25], p1[25]; static plk_fr s0[25], s1[25];
        CK(plk_verify_terms(vk, vk_len, proof, proof_len, 0, p0, s0, &early));
        CK(plk_verify_terms_with(vk, vk_len, proof, proof_len, 0, &kk, p1, s1, &valid));
        WANT(early == 1 && valid == 1 && !memcmp(p0, p1, sizeof p0) && !memcmp(s0, s1, sizeof s0) && open_states == 0, "plk_verify_terms_with under Keccak");
    }
    alt_user u;
    memset(&u, 0, sizeof u);
    plk_transcript_ops alt = alt_ops(&u, 0);
    CK(plk_verify_with(vk, vk_len, proof, proof_len, 0, &alt, &valid));
    WANT(valid == 0 && u.begins == 1 && u.ends == 1, "a Keccak proof under another transcript is invalid, one begin, one end");
    const int calls = u.calls;
    WANT(calls >= 6 && calls <= 29, "the verifier stops at the equation at z or goes to the end");
    for (int k = 1; k <= calls; k++) {                               /* every position fails in turn: an error, one end each */
        memset(&u, 0, sizeof u); u.fail_at = k;
        const int32_t rc = plk_verify_with(vk, vk_len, proof, proof_len, 0, &alt, &valid);
        WANT(rc == PLK_ERR_IO && u.begins == 1 && u.ends == 1 && u.calls == k && strstr(plk_last_error(), "callback (call"), "a failing callback");
    }
    memset(&u, 0, sizeof u); u.big_challenge = 1;
    WANT(plk_verify_with(vk, vk_len, proof, proof_len, 0, &alt, &valid) == PLK_ERR_ARG && u.ends == 1 && strstr(plk_last_error(), "limbs >= r"), "a challenge of r");
    memset(&u, 0, sizeof u);
    WANT(plk_verify_with(vk, vk_len, proof, proof_len - 1, 0, &alt, &valid) == PLK_ERR_ARG && u.begins == 0 && !strcmp(plk_last_error(), "plk_verify: malformed proof"),
         "a truncated proof keeps plk_verify_ex's words and starts no transcript");
    free(vk); free(proof);
    return 0;
}

#ifndef TRANSCRIPT_OPS_HOST_ONLY
#define N_ALT 6
static int gpu_half(void) {
    const uint64_t n = 1024;
    plk_ctx *ctx = 0;
    plk_setup *s = 0;
    plk_vk *key = 0;
    static uint8_t proofs[N_ALT + 3][1 << 12], vk[4096], g2[256];
    uint64_t lens[N_ALT + 3], vk_len = 0;
    alt_user u;
    memset(&u, 0, sizeof u);
    plk_transcript_ops seq = alt_ops(&u, 0), conc = alt_ops(&u, PLK_TRANSCRIPT_CONCURRENT);
    CK(plk_create(0, &ctx));
    CK(plk_srs_generate(ctx, n, 0, 42));
    plk_crs42_g2_bytes(g2);
    for (int k = 0; k < N_ALT + 1; k++) {                            /* one R1CS, a witness per proof; the last one under Keccak */
        plk_circuit *c = 0;
        uint64_t wlen = 0;
        CK(plk_circuit_synthetic_ex(n - 2, 7, (uint64_t)k + 1, 0, &c));
        if (k == 0) { CK(plk_setup_prepare(ctx, c, &s)); CK(plk_setup_write_vk(ctx, s, g2, vk, sizeof vk, &vk_len)); }
        CK(plk_circuit_export(c, 1, 0, 0, &wlen));
        uint8_t *w = (uint8_t *)malloc(wlen);
        if (!w) return 1;
        CK(plk_circuit_export(c, 1, w, wlen, &wlen));
        const uint64_t count = (wlen - 76) / 32;                     /* .wtns: little-endian canonical elements from byte 76 */
        plk_fr *wit = (plk_fr *)malloc(count * sizeof *wit);
        if (!wit) return 1;
        for (uint64_t i = 0; i < count; i++) {
            uint8_t be[32];
            for (int b = 0; b < 32; b++) be[b] = w[76 + 32 * i + 31 - b];
            CK(plk_fr_from_bytes(be, &wit[i]));
        }
        CK(plk_ctx_set_transcript(ctx, k < N_ALT ? &seq : 0));
        CK(plk_prove_witness(ctx, s, wit, count, proofs[k], sizeof proofs[k], &lens[k]));
        free(wit); free(w); plk_circuit_free(c);
    }
    WANT(u.begins == N_ALT && u.ends == N_ALT && u.calls == 26 * N_ALT, "the prover makes 26 calls between begin and end, per proof");
    WANT(lens[0] == lens[1] && memcmp(proofs[0], proofs[1], lens[0]) != 0, "proofs of different witnesses differ");
    memcpy(proofs[N_ALT + 1], proofs[2], lens[2]); lens[N_ALT + 1] = lens[2];
    proofs[N_ALT + 1][lens[2] - 64 - 64 - 1] ^= 1;                   /* the last evaluation, sigma_3(z) */
    memcpy(proofs[N_ALT + 2], proofs[3], lens[3]); lens[N_ALT + 2] = lens[3] - 1;
    const uint8_t *ptrs[N_ALT + 3];
    uint8_t verdict[N_ALT + 3];
    uint64_t first_bad = 0;
    for (int k = 0; k < N_ALT + 3; k++) ptrs[k] = proofs[k];
    CK(plk_vk_load(ctx, vk, vk_len, 0, &key));
    memset(&u, 0, sizeof u);
    CK(plk_verify_many_with(ctx, key, ptrs, lens, N_ALT + 3, &conc, verdict, &first_bad));
    WANT(u.begins == N_ALT + 2 && u.ends == N_ALT + 2, "one begin and one end per well-formed proof");
    for (int k = 0; k < N_ALT + 3; k++) {
        int32_t valid = -1;
        const int32_t rc = plk_verify_with(vk, vk_len, proofs[k], lens[k], 0, &seq, &valid);
        const int want = k < N_ALT ? 1 : (k == N_ALT + 2 ? PLK_VERDICT_MALFORMED : 0);
        WANT((rc == PLK_OK ? valid : PLK_VERDICT_MALFORMED) == want && verdict[k] == want, "verdict of plk_verify_many_with == plk_verify_with");
    }
    WANT(first_bad == N_ALT, "first_bad is the lowest index that is not valid");
    CK(plk_verify_many(ctx, key, ptrs, lens, N_ALT + 3, verdict, &first_bad));
    for (int k = 0; k < N_ALT + 3; k++) WANT(verdict[k] == (k == N_ALT ? 1 : (k == N_ALT + 2 ? PLK_VERDICT_MALFORMED : 0)), "Keccak verdicts of the same batch");
    memset(&u, 0, sizeof u); u.fail_at = 40;                         /* inside the second proof when the front end is sequential */
    WANT(plk_verify_many_with(ctx, key, ptrs, lens, N_ALT + 3, &seq, verdict, &first_bad) == PLK_ERR_IO && u.begins == 2 && u.ends == 2
         && strstr(plk_last_error(), "proof 1: "), "a failing callback ends the batch and names the proof");
    plk_vk_free(key);
    plk_setup_free(s);
    plk_destroy(ctx);
    return 0;
}
#endif

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "host")) { if (host_half(argv[2], argv[3])) return 1; }
#ifndef TRANSCRIPT_OPS_HOST_ONLY
    else if (argc == 2 && !strcmp(argv[1], "gpu")) { if (gpu_half()) return 1; }
#endif
    else { fprintf(stderr, "usage: transcript_ops host vk.bin proof.bin | transcript_ops gpu\n"); return 2; }
    printf("OK %d\n", checks);
    return 0;
}
