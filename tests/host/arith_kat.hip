// Known-answer driver for the header-level primitives (plonkit_amd/csrc/field_dev.h, field29_dev.h, ec_dev.h, ec29_dev.h, ec29_quad_dev.h,
// glv_dev.h, g1_mul_dev.h, msm_shape.h).  It reads a file of cases, applies the named primitive to each case and writes the raw result limbs to an output
// file.  It checks nothing: tests/gen/arith_cases.py owns the cases and the integer model, tests/test_arith_kat_host.py and
// tests/test_gpu_arith_kat.py build this program with hipcc, run it and compare.
//
//     arith_kat [--host] <cases> <results>
//
// With --host the cases are looped over on the CPU (the PLK_HD functions compile for the host too); without it they are copied to the GPU and run
// by one kernel instantiation per primitive (one case per lane, or per quad for the four-lane addition; 256-thread blocks, every lane of the last
// block busy: the case buffers are padded with copies of the last case).  Same dispatch function, same cases, same output format either way.
// The scalar multiplications of g1_mul_dev.h get the dynamic LDS their production kernel (g1ntt_stage) launches with: their window tables live there.
//
// File format, little-endian 32-bit words.  Cases: a sequence of groups { op, field, count, in_words, out_words, count * in_words words }.
// Results: the same groups with count * out_words words each.  field: 0 = Fr / FrW, 1 = Fq / FqW.  Operands are stored limb by limb in the order of
// the function's parameters: Fp = 8 words, W9 = 9 words, Tw3 = 27, XyzzW = x, y, zz, zzz (36 words; NOT the memory layout of store_xyzzw), AffW = 18,
// G1Xyzz = 32, G1Affine = 16, a bool or a 32-bit integer = 1 word, a 64-bit integer = 2.
#include "ec29_quad_dev.h"
#include "glv_dev.h"
#include "g1_mul_dev.h"
#include "msm_shape.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <vector>
using namespace plk;

constexpr int CHAIN_STEPS = 32;

//        name                  id  in   out  fields (1 = Fr, 2 = Fq, 3 = both)  device_only  lanes per case  part (translation unit: KAT_PART)
#define KAT_OPS(X) \
    X(F_ADD,                1,  16,  8,  3, 0, 1, 0) \
    X(F_SUB,                2,  16,  8,  3, 0, 1, 0) \
    X(F_NEG,                3,  8,   8,  3, 0, 1, 0) \
    X(F_DBL,                4,  8,   8,  3, 0, 1, 0) \
    X(F_MUL,                5,  16,  8,  3, 0, 1, 0) \
    X(F_SQR,                6,  8,   8,  3, 0, 1, 0) \
    X(F_INV,                7,  8,   8,  3, 0, 1, 0) \
    X(F_TO_CANONICAL,       8,  8,   8,  3, 0, 1, 0) \
    X(F_FROM_CANONICAL,     9,  8,   8,  3, 0, 1, 0) \
    X(F_FROM_U64,           10, 2,   8,  3, 0, 1, 0) \
    X(F_POW_U64,            11, 10,  8,  3, 0, 1, 0) \
    X(W_MULW,               20, 18,  9,  3, 0, 1, 1) \
    X(W_MULW2,              21, 36,  18, 3, 0, 1, 1) \
    X(W_SQRW,               22, 9,   9,  3, 0, 1, 1) \
    X(W_SQRW2,              23, 18,  18, 3, 0, 1, 1) \
    X(W_MUL2ADDW,           24, 36,  9,  3, 0, 1, 1) \
    X(W_MULSUM3W,           25, 54,  9,  3, 0, 1, 2) \
    X(W_MUL_TW3,            26, 36,  9,  3, 0, 1, 2) \
    X(W_MUL_TW3_2,          27, 45,  18, 3, 0, 1, 2) \
    X(W_MULW_OS,            28, 18,  9,  3, 0, 1, 2) \
    X(W_SQRW_OS,            29, 9,   9,  3, 0, 1, 2) \
    X(W_MUL2ADDW_OS,        30, 36,  9,  3, 0, 1, 2) \
    X(W_SUB2,               31, 18,  9,  3, 0, 1, 3) \
    X(W_SUB4,               32, 18,  9,  3, 0, 1, 3) \
    X(W_SUB6,               33, 18,  9,  3, 0, 1, 3) \
    X(W_NEG2,               34, 9,   9,  3, 0, 1, 3) \
    X(W_NORMW,              35, 9,   9,  3, 0, 1, 3) \
    X(W_CSUB_P,             36, 9,   9,  3, 0, 1, 3) \
    X(W_REDUCE_FULL,        37, 9,   9,  3, 0, 1, 3) \
    X(W_REDUCE_SMALL,       38, 9,   9,  3, 0, 1, 3) \
    X(W_IS_ZERO_MOD_P,      39, 9,   1,  3, 0, 1, 3) \
    X(W_MAYBE_ZERO_MOD_P,   40, 9,   1,  3, 0, 1, 3) \
    X(W_UNPACK,             41, 8,   9,  3, 0, 1, 3) \
    X(W_PACK,               42, 9,   8,  3, 0, 1, 3) \
    X(W_W_FROM_S,           43, 9,   9,  3, 0, 1, 3) \
    X(W_S_FROM_W,           44, 9,   9,  3, 0, 1, 3) \
    X(E_XYZZ_ADD_MIXED,     60, 49,  32, 2, 0, 1, 4) \
    X(E_XYZZ_ADD,           61, 64,  32, 2, 0, 1, 4) \
    X(E_XYZZ_DOUBLE,        62, 32,  32, 2, 0, 1, 4) \
    X(E_XYZZW_ADD_MIXED,    63, 55,  36, 2, 0, 1, 5) \
    X(E_XYZZW_ADD,          64, 72,  36, 2, 0, 1, 6) \
    X(E_XYZZW_DOUBLE,       65, 36,  36, 2, 0, 1, 4) \
    X(E_XYZZW_DOUBLE_AFFINE, 66, 18, 36, 2, 0, 1, 4) \
    X(E_XYZZW_ADD_MIXED_SPECIAL, 67, 73, 36, 2, 0, 1, 5) \
    X(E_XYZZW_CHAIN,        68, 140, 36 * CHAIN_STEPS, 2, 0, 1, 7) \
    X(E_XYZZW_EXPORT,       69, 36,  32, 2, 1, 1, 6) \
    X(E_XYZZW_STORE_LOAD,   70, 36,  72, 2, 1, 1, 6) \
    X(Q_ADD_DIST,           71, 72,  36, 2, 1, 4, 8) \
    X(Q_DISTRIBUTE_GATHER0, 72, 144, 144, 2, 1, 4, 8) \
    X(Q_DISTRIBUTE_GATHER1, 73, 144, 144, 2, 1, 4, 8) \
    X(Q_DISTRIBUTE_GATHER2, 74, 144, 144, 2, 1, 4, 8) \
    X(Q_DISTRIBUTE_GATHER3, 75, 144, 144, 2, 1, 4, 8) \
    X(E_XYZZW_ADD_MIXED_OS, 76, 55,  36, 2, 0, 1, 3) \
    X(G_GLV_SPLIT,          80, 8,   12, 1, 0, 1, 8) \
    X(G_GLV_DIGITS,         81, 5,   6,  1, 0, 1, 8) \
    X(G_GLV_DIGITS4,        82, 5,   6,  1, 0, 1, 8) \
    X(G_RECODE17,           83, 8,   15, 1, 0, 1, 8) \
    X(G_EXTRACT_BITS,       84, 10,  1,  1, 0, 1, 8) \
    X(G_MUL_SCALAR,         85, 44,  36, 2, 1, 1, 9) \
    X(G_MUL_SCALAR_ISO,     86, 44,  36, 2, 1, 1, 10) \
    X(G_MUL_SCALAR_ISO8,    87, 44,  36, 2, 1, 1, 11)

enum OpId : uint32_t {
#define X(name, id, in_w, out_w, fields, dev_only, lanes, part) name = id,
    KAT_OPS(X)
#undef X
};

// ---- operands <-> words
template <class PR> PLK_HD Fp<PR> get_f(const uint32_t *p) { Fp<PR> r; for (int i = 0; i < 8; i++) r.l[i] = p[i]; return r; }
template <class PR> PLK_HD void put_f(uint32_t *p, const Fp<PR> &v) { for (int i = 0; i < 8; i++) p[i] = v.l[i]; }
template <class WP> PLK_HD W9<WP> get_w(const uint32_t *p) { W9<WP> r; for (int i = 0; i < 9; i++) r.l[i] = p[i]; return r; }
template <class WP> PLK_HD void put_w(uint32_t *p, const W9<WP> &v) { for (int i = 0; i < 9; i++) p[i] = v.l[i]; }
template <class WP> PLK_HD Tw3<WP> get_tw3(const uint32_t *p) { Tw3<WP> t; for (int q = 0; q < 3; q++) for (int i = 0; i < 9; i++) t.w[q][i] = p[9 * q + i]; return t; }
PLK_HD XyzzW get_xw(const uint32_t *p) { XyzzW r; r.x = get_w<FqW>(p); r.y = get_w<FqW>(p + 9); r.zz = get_w<FqW>(p + 18); r.zzz = get_w<FqW>(p + 27); return r; }
PLK_HD void put_xw(uint32_t *p, const XyzzW &v) { put_w(p, v.x); put_w(p + 9, v.y); put_w(p + 18, v.zz); put_w(p + 27, v.zzz); }
PLK_HD AffW get_aw(const uint32_t *p) { AffW r; r.x = get_w<FqW>(p); r.y = get_w<FqW>(p + 9); return r; }
PLK_HD G1Xyzz get_x(const uint32_t *p) { G1Xyzz r; r.x = get_f<FqParams>(p); r.y = get_f<FqParams>(p + 8); r.zz = get_f<FqParams>(p + 16); r.zzz = get_f<FqParams>(p + 24); return r; }
PLK_HD void put_x(uint32_t *p, const G1Xyzz &v) { put_f(p, v.x); put_f(p + 8, v.y); put_f(p + 16, v.zz); put_f(p + 24, v.zzz); }
PLK_HD G1Affine get_a(const uint32_t *p) { G1Affine r; r.x = get_f<FqParams>(p); r.y = get_f<FqParams>(p + 8); return r; }

// ---- THE dispatch function: one primitive applied to one case.  OP is a template parameter, so every kernel holds one primitive.
// `in` / `out`: this case's words (for a four-lane primitive: the quad's case, shared by its lanes); `mem`: 72 words of global memory of this
// lane's own, 16-byte aligned; role: lane & 3 (four-lane primitives only); lds: the block's dynamic shared memory (lds_bytes<OP>() of it).
template <uint32_t OP, class PR, class WP>
PLK_HD void apply(const uint32_t *in, uint32_t *out, uint32_t *mem, uint32_t role, uint32_t *lds) {
    (void)mem; (void)role; (void)lds;
    // ---- field_dev.h
    if constexpr (OP == F_ADD) put_f(out, add(get_f<PR>(in), get_f<PR>(in + 8)));
    else if constexpr (OP == F_SUB) put_f(out, sub(get_f<PR>(in), get_f<PR>(in + 8)));
    else if constexpr (OP == F_NEG) put_f(out, neg(get_f<PR>(in)));
    else if constexpr (OP == F_DBL) put_f(out, dbl(get_f<PR>(in)));
    else if constexpr (OP == F_MUL) put_f(out, mul(get_f<PR>(in), get_f<PR>(in + 8)));
    else if constexpr (OP == F_SQR) put_f(out, sqr(get_f<PR>(in)));
    else if constexpr (OP == F_INV) put_f(out, inv(get_f<PR>(in)));
    else if constexpr (OP == F_TO_CANONICAL) put_f(out, to_canonical(get_f<PR>(in)));
    else if constexpr (OP == F_FROM_CANONICAL) put_f(out, from_canonical(get_f<PR>(in)));
    else if constexpr (OP == F_FROM_U64) put_f(out, from_u64<PR>((uint64_t)in[0] | ((uint64_t)in[1] << 32)));
    else if constexpr (OP == F_POW_U64) put_f(out, pow_u64(get_f<PR>(in), (uint64_t)in[8] | ((uint64_t)in[9] << 32)));
    // ---- field29_dev.h
    else if constexpr (OP == W_MULW) put_w(out, mulw(get_w<WP>(in), get_w<WP>(in + 9)));
    else if constexpr (OP == W_MULW2) { W9<WP> r0, r1; mulw2(get_w<WP>(in), get_w<WP>(in + 9), get_w<WP>(in + 18), get_w<WP>(in + 27), r0, r1); put_w(out, r0); put_w(out + 9, r1); }
    else if constexpr (OP == W_SQRW) put_w(out, sqrw(get_w<WP>(in)));
    else if constexpr (OP == W_SQRW2) { W9<WP> r0, r1; sqrw2(get_w<WP>(in), get_w<WP>(in + 9), r0, r1); put_w(out, r0); put_w(out + 9, r1); }
    else if constexpr (OP == W_MUL2ADDW) put_w(out, mul2addw(get_w<WP>(in), get_w<WP>(in + 9), get_w<WP>(in + 18), get_w<WP>(in + 27)));
    else if constexpr (OP == W_MULSUM3W) put_w(out, mulsum3w(get_w<WP>(in), get_w<WP>(in + 9), get_w<WP>(in + 18), get_w<WP>(in + 27), get_w<WP>(in + 36), get_w<WP>(in + 45)));
    else if constexpr (OP == W_MUL_TW3) put_w(out, mul_tw3(get_w<WP>(in), get_tw3<WP>(in + 9)));
    else if constexpr (OP == W_MUL_TW3_2) { W9<WP> r0, r1; mul_tw3_2(get_w<WP>(in), get_w<WP>(in + 9), get_tw3<WP>(in + 18), r0, r1); put_w(out, r0); put_w(out + 9, r1); }
    else if constexpr (OP == W_MULW_OS) put_w(out, mulw_os(get_w<WP>(in), get_w<WP>(in + 9)));
    else if constexpr (OP == W_SQRW_OS) put_w(out, sqrw_os(get_w<WP>(in)));
    else if constexpr (OP == W_MUL2ADDW_OS) put_w(out, mul2addw_os(get_w<WP>(in), get_w<WP>(in + 9), get_w<WP>(in + 18), get_w<WP>(in + 27)));
    else if constexpr (OP == W_SUB2) put_w(out, sub2(get_w<WP>(in), get_w<WP>(in + 9)));
    else if constexpr (OP == W_SUB4) put_w(out, sub4(get_w<WP>(in), get_w<WP>(in + 9)));
    else if constexpr (OP == W_SUB6) put_w(out, sub6(get_w<WP>(in), get_w<WP>(in + 9)));
    else if constexpr (OP == W_NEG2) put_w(out, neg2(get_w<WP>(in)));
    else if constexpr (OP == W_NORMW) put_w(out, normw(get_w<WP>(in)));
    else if constexpr (OP == W_CSUB_P) put_w(out, csub_p(get_w<WP>(in)));
    else if constexpr (OP == W_REDUCE_FULL) put_w(out, reduce_full(get_w<WP>(in)));
    else if constexpr (OP == W_REDUCE_SMALL) put_w(out, reduce_small(get_w<WP>(in)));
    else if constexpr (OP == W_IS_ZERO_MOD_P) out[0] = is_zero_mod_p(get_w<WP>(in)) ? 1u : 0u;
    else if constexpr (OP == W_MAYBE_ZERO_MOD_P) out[0] = maybe_zero_mod_p(get_w<WP>(in)) ? 1u : 0u;
    else if constexpr (OP == W_UNPACK) put_w(out, unpack<WP>(get_f<PR>(in)));
    else if constexpr (OP == W_PACK) put_f(out, pack<PR>(get_w<WP>(in)));
    else if constexpr (OP == W_W_FROM_S) put_w(out, w_from_s(get_w<WP>(in)));
    else if constexpr (OP == W_S_FROM_W) put_w(out, s_from_w(get_w<WP>(in)));
    // ---- ec_dev.h
    else if constexpr (OP == E_XYZZ_ADD_MIXED) { G1Xyzz acc = get_x(in); xyzz_add_mixed(acc, get_a(in + 32), in[48] != 0); put_x(out, acc); }
    else if constexpr (OP == E_XYZZ_ADD) { G1Xyzz a = get_x(in); xyzz_add(a, get_x(in + 32)); put_x(out, a); }
    else if constexpr (OP == E_XYZZ_DOUBLE) put_x(out, xyzz_double(get_x(in)));
    // ---- ec29_dev.h
    else if constexpr (OP == E_XYZZW_ADD_MIXED) { XyzzW acc = get_xw(in); xyzzw_add_mixed(acc, get_aw(in + 36), in[54] != 0); put_xw(out, acc); }
    else if constexpr (OP == E_XYZZW_ADD) { XyzzW a = get_xw(in); xyzzw_add(a, get_xw(in + 36)); put_xw(out, a); }
    else if constexpr (OP == E_XYZZW_DOUBLE) put_xw(out, xyzzw_double(get_xw(in)));
    else if constexpr (OP == E_XYZZW_DOUBLE_AFFINE) put_xw(out, xyzzw_double_affine(get_w<FqW>(in), get_w<FqW>(in + 9)));
    else if constexpr (OP == E_XYZZW_ADD_MIXED_SPECIAL) {
        XyzzW acc = get_xw(in);
        xyzzw_add_mixed_special(acc, get_aw(in + 36), in[54] != 0, get_w<FqW>(in + 55), get_w<FqW>(in + 64));
        put_xw(out, acc);
    }
    // ---- g1_mul_dev.h
    else if constexpr (OP == E_XYZZW_ADD_MIXED_OS) { XyzzW acc = get_xw(in); xyzzw_add_mixed_os(acc, get_aw(in + 36), in[54] != 0); put_xw(out, acc); }
    else if constexpr (OP == E_XYZZW_CHAIN) {                      // acc | affine 0 | affine 1 | xyzz | 32 schedule words; every intermediate result is written
        XyzzW acc = get_xw(in);
        const AffW a0 = get_aw(in + 36), a1 = get_aw(in + 54);
        const XyzzW b = get_xw(in + 72);
        for (int s = 0; s < CHAIN_STEPS; s++) {
            const uint32_t o = in[108 + s];                         // 0..3: acc += +-affine (bit 1: which, bit 0: negated); 4: doubling; 5: acc += xyzz
            if (o < 4) xyzzw_add_mixed(acc, (o & 2) ? a1 : a0, (o & 1) != 0);
            else if (o == 4) acc = xyzzw_double(acc);
            else xyzzw_add(acc, b);
            put_xw(out + 36 * s, acc);
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
    // ---- __device__-only: the device run covers them, the host run cannot
    else if constexpr (OP == E_XYZZW_EXPORT) put_x(out, xyzzw_export(get_xw(in)));
    else if constexpr (OP == E_XYZZW_STORE_LOAD) {                  // out: the point as load_xyzzw returns it | the 36 words store_xyzzw left in memory
        store_xyzzw(reinterpret_cast<XyzzW *>(mem), get_xw(in));
        __threadfence();
        put_xw(out, load_xyzzw(reinterpret_cast<const XyzzW *>(mem)));
        for (int i = 0; i < 36; i++) out[36 + i] = mem[i];
    }
    // ---- ec29_quad_dev.h: a case per quad; lane `role` holds coordinate `role`
    else if constexpr (OP == Q_ADD_DIST) {
        const FqW9 r = xyzzw_add_dist(get_w<FqW>(in + 9 * role), get_w<FqW>(in + 36 + 9 * role), role);
        put_w(out + 9 * role, r);
    }
    else if constexpr (OP >= Q_DISTRIBUTE_GATHER0 && OP <= Q_DISTRIBUTE_GATHER3) {   // lane r holds point r in full; every lane must end up with lane SRC's
        const XyzzW mine = get_xw(in + 36 * role);
        put_xw(out + 36 * role, quad_gather(quad_distribute<(int)(OP - Q_DISTRIBUTE_GATHER0)>(mine, role)));
    }
    // ---- g1_mul_dev.h: the base | a canonical scalar below r; the window table of the lane is in the block's LDS, as in g1ntt_stage
    else if constexpr (OP == G_MUL_SCALAR) put_xw(out, g1_mul_scalar(get_xw(in), get_f<FrParams>(in + 36), lds));
    else if constexpr (OP == G_MUL_SCALAR_ISO) put_xw(out, g1_mul_scalar_iso(get_xw(in), get_f<FrParams>(in + 36), lds));
    else if constexpr (OP == G_MUL_SCALAR_ISO8) put_xw(out, g1_mul_scalar_iso8(get_xw(in), get_f<FrParams>(in + 36), lds));
#endif
    // ---- glv_dev.h, msm_shape.h
    else if constexpr (OP == G_GLV_SPLIT) {
        uint32_t k[8];
        for (int i = 0; i < 8; i++) k[i] = in[i];
        const GlvSplit s = glv_split(k);
        for (int i = 0; i < 5; i++) { out[i] = s.k1[i]; out[5 + i] = s.k2[i]; }
        out[10] = s.neg1 ? 1u : 0u; out[11] = s.neg2 ? 1u : 0u;
    }
    else if constexpr (OP == G_GLV_DIGITS || OP == G_GLV_DIGITS4) {
        uint32_t k[5], d[6];
        for (int i = 0; i < 5; i++) k[i] = in[i];
        if constexpr (OP == G_GLV_DIGITS) glv_digits(k, d); else glv_digits4(k, d);
        for (int i = 0; i < 6; i++) out[i] = d[i];
    }
    else if constexpr (OP == G_RECODE17) {
        int32_t d[RC_WINDOWS];
        recode17(get_f<FrParams>(in), d);
        for (int i = 0; i < RC_WINDOWS; i++) out[i] = (uint32_t)d[i];
    }
    else if constexpr (OP == G_EXTRACT_BITS) {
        uint32_t k[8];
        for (int i = 0; i < 8; i++) k[i] = in[i];
        out[0] = extract_bits(k, in[8], in[9]);
    }
}

// dynamic LDS of a block: what g1_intt_dev launches g1ntt_stage with for the same multiplication (256 lanes wide: G1NTT_THREADS)
template <uint32_t OP> constexpr size_t lds_bytes() {
    return OP == G_MUL_SCALAR ? G1NTT_LDS : OP == G_MUL_SCALAR_ISO ? G1NTT_LDS_ISO : OP == G_MUL_SCALAR_ISO8 ? G1NTT_LDS_ISO8 : 0;
}
static_assert(G1NTT_THREADS == 256, "the kernels below are launched with 256-thread blocks");

// n_padded cases (a multiple of 256 / LANES), all of them real work: no lane idles and none leaves early
template <uint32_t OP, class PR, class WP, uint32_t IN_W, uint32_t OUT_W, uint32_t LANES>
__global__ void __launch_bounds__(256) kat_kernel(const uint32_t *in, uint32_t *out, uint32_t *mem) {
    extern __shared__ uint32_t kat_lds[];
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x, c = tid / LANES;
    apply<OP, PR, WP>(in + (size_t)c * IN_W, out + (size_t)c * OUT_W, mem + (size_t)tid * 72u, tid % LANES, kat_lds);
}

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "arith_kat: %s failed: %s\n", #call, hipGetErrorString(e_)); exit(3); } } while (0)

template <uint32_t OP, class PR, class WP, uint32_t IN_W, uint32_t OUT_W, uint32_t LANES>
static void run_device(const uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t per_block = 256u / LANES, blocks = (n + per_block - 1) / per_block, n_pad = blocks * per_block;
    std::vector<uint32_t> h_in((size_t)n_pad * IN_W);
    memcpy(h_in.data(), in, (size_t)n * IN_W * 4);
    for (uint32_t i = n; i < n_pad; i++) memcpy(&h_in[(size_t)i * IN_W], in + (size_t)(n - 1) * IN_W, IN_W * 4);
    std::vector<uint32_t> h_out((size_t)n_pad * OUT_W);
    uint32_t *d_in, *d_out, *d_mem;
    CK(hipMalloc(&d_in, h_in.size() * 4));
    CK(hipMalloc(&d_out, h_out.size() * 4));
    CK(hipMalloc(&d_mem, (size_t)blocks * 256 * 72 * 4));
    CK(hipMemcpy(d_in, h_in.data(), h_in.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xee, h_out.size() * 4));
    CK(hipMemset(d_mem, 0xee, (size_t)blocks * 256 * 72 * 4));
    constexpr size_t lds = lds_bytes<OP>();
    if constexpr (lds > 64 * 1024)                               // above the default limit of a launch: raised as g1_intt_dev does
        CK(hipFuncSetAttribute(reinterpret_cast<const void *>(kat_kernel<OP, PR, WP, IN_W, OUT_W, LANES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((kat_kernel<OP, PR, WP, IN_W, OUT_W, LANES>), dim3(blocks), dim3(256), lds, 0, d_in, d_out, d_mem);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_out.data(), d_out, h_out.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(d_in)); CK(hipFree(d_out)); CK(hipFree(d_mem));
    memcpy(out, h_out.data(), (size_t)n * OUT_W * 4);
}

template <uint32_t OP, class PR, class WP, uint32_t IN_W, uint32_t OUT_W>
static void run_host(const uint32_t *in, uint32_t *out, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) apply<OP, PR, WP>(in + (size_t)i * IN_W, out + (size_t)i * OUT_W, nullptr, 0, nullptr);
}

struct Entry {
    const char *name;
    uint32_t op, field, in_w, out_w;
    void (*host)(const uint32_t *, uint32_t *, uint32_t);
    void (*dev)(const uint32_t *, uint32_t *, uint32_t);
};
template <uint32_t OP, class PR, class WP, uint32_t IN_W, uint32_t OUT_W, uint32_t LANES, bool DEV_ONLY>
static Entry entry(const char *name, uint32_t field) {
    Entry e{name, OP, field, IN_W, OUT_W, nullptr, &run_device<OP, PR, WP, IN_W, OUT_W, LANES>};
    if constexpr (!DEV_ONLY) e.host = &run_host<OP, PR, WP, IN_W, OUT_W>;
    return e;
}

// The primitives are spread over KAT_PARTS translation units so that the tests can compile them side by side: hipcc -DKAT_PART=<k> -c builds the
// kernels and host loops of part k alone, -DKAT_MAIN -c builds main(), and the objects link into one program.  With neither macro the whole program
// is one translation unit.
constexpr int KAT_PARTS = 12;
template <int PART>
static void add_part(std::vector<Entry> &t) {
#define X(name, id, in_w, out_w, fields, dev_only, lanes, part) \
    if constexpr ((part) == PART && ((fields) & 1) != 0) t.push_back(entry<name, FrParams, FrW, in_w, out_w, lanes, dev_only != 0>(#name, 0)); \
    if constexpr ((part) == PART && ((fields) & 2) != 0) t.push_back(entry<name, FqParams, FqW, in_w, out_w, lanes, dev_only != 0>(#name, 1));
    KAT_OPS(X)
#undef X
}
#define KAT_CAT2(a, b) a##b
#define KAT_CAT(a, b) KAT_CAT2(a, b)
#if defined(KAT_PART)
void KAT_CAT(kat_add_part_, KAT_PART)(std::vector<Entry> &t) { add_part<KAT_PART>(t); }
#else
#if defined(KAT_MAIN)
void kat_add_part_0(std::vector<Entry> &t); void kat_add_part_1(std::vector<Entry> &t); void kat_add_part_2(std::vector<Entry> &t);
void kat_add_part_3(std::vector<Entry> &t); void kat_add_part_4(std::vector<Entry> &t); void kat_add_part_5(std::vector<Entry> &t);
void kat_add_part_6(std::vector<Entry> &t); void kat_add_part_7(std::vector<Entry> &t); void kat_add_part_8(std::vector<Entry> &t);
void kat_add_part_9(std::vector<Entry> &t); void kat_add_part_10(std::vector<Entry> &t); void kat_add_part_11(std::vector<Entry> &t);
static std::vector<Entry> table() {
    std::vector<Entry> t;
    kat_add_part_0(t); kat_add_part_1(t); kat_add_part_2(t); kat_add_part_3(t); kat_add_part_4(t); kat_add_part_5(t); kat_add_part_6(t); kat_add_part_7(t); kat_add_part_8(t);
    kat_add_part_9(t); kat_add_part_10(t); kat_add_part_11(t);
    return t;
}
#else
template <int... K> static void add_parts(std::vector<Entry> &t, std::integer_sequence<int, K...>) { (add_part<K>(t), ...); }
static std::vector<Entry> table() { std::vector<Entry> t; add_parts(t, std::make_integer_sequence<int, KAT_PARTS>{}); return t; }
#endif

int main(int argc, char **argv) {
    bool host = false;
    std::vector<const char *> paths;
    for (int i = 1; i < argc; i++) { if (!strcmp(argv[i], "--host")) host = true; else paths.push_back(argv[i]); }
    if (paths.size() != 2) { fprintf(stderr, "usage: arith_kat [--host] <cases> <results>\n"); return 2; }
    FILE *f = fopen(paths[0], "rb");
    if (!f) { fprintf(stderr, "arith_kat: cannot read %s\n", paths[0]); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> cases((size_t)bytes / 4);
    if (bytes % 4 || fread(cases.data(), 1, (size_t)bytes, f) != (size_t)bytes) { fprintf(stderr, "arith_kat: short read\n"); return 2; }
    fclose(f);
    FILE *o = fopen(paths[1], "wb");
    if (!o) { fprintf(stderr, "arith_kat: cannot write %s\n", paths[1]); return 2; }
    const std::vector<Entry> t = table();
    size_t pos = 0, groups = 0, total = 0;
    const auto t0 = std::chrono::steady_clock::now();
    while (pos < cases.size()) {
        if (pos + 5 > cases.size()) { fprintf(stderr, "arith_kat: truncated group header\n"); return 2; }
        const uint32_t op = cases[pos], field = cases[pos + 1], n = cases[pos + 2], in_w = cases[pos + 3], out_w = cases[pos + 4];
        const Entry *e = nullptr;
        for (const Entry &c : t) if (c.op == op && c.field == field) e = &c;
        if (!e || e->in_w != in_w || e->out_w != out_w || n == 0 || pos + 5 + (size_t)n * in_w > cases.size()) {
            fprintf(stderr, "arith_kat: bad group (op %u field %u count %u in %u out %u)\n", op, field, n, in_w, out_w); return 2;
        }
        if (host && !e->host) { fprintf(stderr, "arith_kat: %s is __device__ only\n", e->name); return 2; }
        std::vector<uint32_t> out((size_t)n * out_w);
        if (host) e->host(&cases[pos + 5], out.data(), n); else e->dev(&cases[pos + 5], out.data(), n);
        if (fwrite(&cases[pos], 4, 5, o) != 5 || fwrite(out.data(), 4, out.size(), o) != out.size()) { fprintf(stderr, "arith_kat: write failed\n"); return 2; }
        pos += 5 + (size_t)n * in_w;
        groups++; total += n;
    }
    if (fclose(o) != 0) { fprintf(stderr, "arith_kat: write failed\n"); return 2; }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("arith_kat: %zu groups, %zu cases on the %s in %.1f ms\n", groups, total, host ? "host" : "device", ms);
    return 0;
}
#endif
