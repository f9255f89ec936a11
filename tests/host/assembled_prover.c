/* A proof from setup polynomials and assembled wire columns through the C ABI alone (no Python in the proving process): what a Rust
 * host that holds bellman's SetupPolynomials and the prover assembly's columns would do (src/plonk.rs:50-55,104,
 * 152-159).  Reads, from the directory given as the first argument, raw little-endian files of 32-byte Montgomery Fr elements —
 * q_a q_b q_c q_d q_m q_const q_d_next sigma_1 .. sigma_4 (coefficient form, equal length) and column_a .. column_d (equal length,
 * the rows) — plus key_points (64-byte affine G1 points) and key_g2 (the key file's 256-byte G2 section), and writes vk.bin and
 * proof.bin there.  Built and run by tests/test_gpu_assembled.py:
 *   gcc -std=c99 -O2 -I include tests/host/assembled_prover.c -L plonkit_amd/lib -lplonkit_amd -Wl,-rpath,$PWD/plonkit_amd/lib
 *   ./a.out <dir> <n> <num_inputs>                                                                                                  */
#include "plonkit_amd.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CK(x) do { int32_t rc_ = (x); if (rc_ != PLK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, plk_last_error()); return 1; } } while (0)

static void *read_file(const char *dir, const char *name, size_t *len) {
    char path[4096];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(1); }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    void *p = malloc(n > 0 ? (size_t)n : 1);
    if (!p || fread(p, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot read %s\n", path); exit(1); }
    fclose(f);
    *len = (size_t)n;
    return p;
}

static int write_file(const char *dir, const char *name, const uint8_t *p, uint64_t len) {
    char path[4096];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, len, f) != len) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    return fclose(f) != 0;
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s <dir> <n> <num_inputs>\n", argv[0]); return 2; }
    const char *dir = argv[1];
    const uint64_t n = strtoull(argv[2], 0, 10), num_inputs = strtoull(argv[3], 0, 10);
    static const char *const polys[11] = {"q_a", "q_b", "q_c", "q_d", "q_m", "q_const", "q_d_next", "sigma_1", "sigma_2", "sigma_3", "sigma_4"};
    static const char *const cols[4] = {"column_a", "column_b", "column_c", "column_d"};
    const plk_fr *v[11], *c[4];
    size_t len = 0, rows = 0, bytes = 0;
    for (int i = 0; i < 11; i++) {
        v[i] = read_file(dir, polys[i], &bytes);
        if (i && bytes != len * sizeof(plk_fr)) { fprintf(stderr, "%s: length differs\n", polys[i]); return 1; }
        len = bytes / sizeof(plk_fr);
    }
    for (int j = 0; j < 4; j++) {
        c[j] = read_file(dir, cols[j], &bytes);
        if (j && bytes != rows * sizeof(plk_fr)) { fprintf(stderr, "%s: length differs\n", cols[j]); return 1; }
        rows = bytes / sizeof(plk_fr);
    }
    const plk_g1_affine *pts = read_file(dir, "key_points", &bytes);
    const uint64_t npts = bytes / sizeof(plk_g1_affine);
    const uint8_t *g2 = read_file(dir, "key_g2", &bytes);
    if (bytes != 256) { fprintf(stderr, "key_g2: 256 bytes expected\n"); return 1; }

    plk_ctx *ctx = 0;
    CK(plk_create(0, &ctx));
    CK(plk_srs_upload(ctx, pts, npts));
    plk_setup *s = 0;
    const plk_fr *const sel[6] = {v[0], v[1], v[2], v[3], v[4], v[5]};
    const plk_fr *const sig[4] = {v[7], v[8], v[9], v[10]};
    CK(plk_setup_from_polynomials(ctx, n, num_inputs, sel, v[6], sig, len, 0, &s));
    if (plk_setup_domain_size(s) != n + 1) { fprintf(stderr, "domain size %llu\n", (unsigned long long)plk_setup_domain_size(s)); return 1; }
    static uint8_t vk[4096], proof[1 << 16];
    uint64_t vk_len = 0, proof_len = 0;
    CK(plk_setup_write_vk(ctx, s, g2, vk, sizeof vk, &vk_len));
    CK(plk_prove_assembled(ctx, s, c, rows, proof, sizeof proof, &proof_len));
    int32_t valid = 0;
    CK(plk_verify(vk, vk_len, proof, proof_len, &valid));
    if (!valid) { fprintf(stderr, "the host verifier rejects the proof\n"); return 1; }
    if (write_file(dir, "vk.bin", vk, vk_len) || write_file(dir, "proof.bin", proof, proof_len)) return 1;
    plk_setup_free(s);
    plk_destroy(ctx);
    for (int i = 0; i < 11; i++) free((void *)v[i]);
    for (int j = 0; j < 4; j++) free((void *)c[j]);
    free((void *)pts); free((void *)g2);
    printf("OK %llu %llu\n", (unsigned long long)vk_len, (unsigned long long)proof_len);
    return 0;
}
