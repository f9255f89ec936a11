// The front end of the PLONK verifier as host + device code: proof bytes -> (state, the proof's 11 points, the 25 flattened scalars).
// NO COUNTERPART IN THE REFERENCE as device code; it restates, line for line, what verify.cpp runs on the host per proof before any group
// arithmetic: parse_proof / Reader / g1_from_bytes (hostapi.cpp), RollingKeccak (hostapi.cpp:70-100) and flatten_keccak (verify.cpp).
// Everything is __host__ __device__ (tests/host/verify_front_check.hip runs the same code on the CPU against those functions); one proof
// per lane on the device (verify_front.hip).
//
// Keccak.  Every message of the rolling transcript is a single rate block (100 bytes for an absorbed word, 72 for a challenge), so the
// sponge is one permutation of a block that is built directly as 64-bit lanes from the state words and the big-endian word — no byte
// buffer.  The 25 lanes are named with compile-time indices only (theta, rho / pi and chi are written out), so they stay in registers; the
// permutation exists ONCE per kernel, behind keccak256_padded (out of line on the device), and its 24 rounds run as 6 trips of 4: the whole
// of it unrolled is ~50 KB of code for an instruction cache of 64 KB that two CUs share (the reason ec_dev.h keeps one Montgomery product).
//
// Field products go through one out-of-line copy each (ECM for Fq, FRM for Fr), for the same reason.
#pragma once
#include "ec_dev.h"
#include "verify_front.h"

namespace plk {

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __noinline__ Fr fr_mul_call(Fr a, Fr b) { return plk::mul<FrParams>(a, b); }
#define FRM(a, b) fr_mul_call((a), (b))
#define PLK_HD_CALL __host__ __device__ __noinline__
#else
#define FRM(a, b) plk::mul((a), (b))
#define PLK_HD_CALL __host__ __device__ inline
#endif

PLK_HD Fr to_canonical_call(const Fr &a) { Fr o = Fr::zero(); o.l[0] = 1; return FRM(a, o); }
PLK_HD Fr fr_from_u64_call(uint64_t v) { Fr o = Fr::zero(); o.l[0] = (uint32_t)v; o.l[1] = (uint32_t)(v >> 32); return FRM(o, Fr::r2()); }
PLK_HD Fq fq_from_u64_call(uint64_t v) { Fq o = Fq::zero(); o.l[0] = (uint32_t)v; o.l[1] = (uint32_t)(v >> 32); return ECM(o, Fq::r2()); }

// ---------------------------------------------------------------------------------------------- Keccak-f[1600], Keccak-256 of one block
PLK_HD uint64_t kf_rotl(uint64_t x, int s) { return (x << s) | (x >> (64 - s)); }      // 0 < s < 64

PLK_HD uint64_t kf_round_constant(int r) {
    constexpr uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL, 0x0000000080000001ULL,
        0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
        0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
        0x000000000000800aULL, 0x800000008000000aULL, 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    return RC[r];
}

// one round on lanes a[x + 5 y]; every index is a literal
PLK_HD void kf_round(uint64_t (&a)[25], uint64_t rc) {
    const uint64_t c0 = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20], c1 = a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21], c2 = a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22],
                   c3 = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23], c4 = a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24];
    const uint64_t d0 = c4 ^ kf_rotl(c1, 1), d1 = c0 ^ kf_rotl(c2, 1), d2 = c1 ^ kf_rotl(c3, 1), d3 = c2 ^ kf_rotl(c4, 1), d4 = c3 ^ kf_rotl(c0, 1);
    uint64_t b[25];
    // rho and pi: lane (x, y) rotated by its offset lands on (y, 2x + 3y)
#define KF_RP(dst, src, d, rot) b[dst] = kf_rotl(a[src] ^ d, rot)
    b[0] = a[0] ^ d0;
    KF_RP(10, 1, d1, 1);   KF_RP(20, 2, d2, 62);  KF_RP(5, 3, d3, 28);   KF_RP(15, 4, d4, 27);
    KF_RP(16, 5, d0, 36);  KF_RP(1, 6, d1, 44);   KF_RP(11, 7, d2, 6);   KF_RP(21, 8, d3, 55);  KF_RP(6, 9, d4, 20);
    KF_RP(7, 10, d0, 3);   KF_RP(17, 11, d1, 10); KF_RP(2, 12, d2, 43);  KF_RP(12, 13, d3, 25); KF_RP(22, 14, d4, 39);
    KF_RP(23, 15, d0, 41); KF_RP(8, 16, d1, 45);  KF_RP(18, 17, d2, 15); KF_RP(3, 18, d3, 21);  KF_RP(13, 19, d4, 8);
    KF_RP(14, 20, d0, 18); KF_RP(24, 21, d1, 2);  KF_RP(9, 22, d2, 61);  KF_RP(19, 23, d3, 56); KF_RP(4, 24, d4, 14);
#undef KF_RP
#define KF_CHI(y)                                                                                                                              \
    a[y] = b[y] ^ (~b[y + 1] & b[y + 2]); a[y + 1] = b[y + 1] ^ (~b[y + 2] & b[y + 3]); a[y + 2] = b[y + 2] ^ (~b[y + 3] & b[y + 4]);            \
    a[y + 3] = b[y + 3] ^ (~b[y + 4] & b[y]); a[y + 4] = b[y + 4] ^ (~b[y] & b[y + 1])
    KF_CHI(0); KF_CHI(5); KF_CHI(10); KF_CHI(15); KF_CHI(20);
#undef KF_CHI
    a[0] ^= rc;
}

PLK_HD void keccak_f1600(uint64_t (&a)[25]) {
#pragma unroll 1
    for (int r = 0; r < 24; r += 4) {
        kf_round(a, kf_round_constant(r)); kf_round(a, kf_round_constant(r + 1));
        kf_round(a, kf_round_constant(r + 2)); kf_round(a, kf_round_constant(r + 3));
    }
}

// Keccak-256 of ONE rate block that already carries its padding: m = the 17 little-endian lanes of message | 0x01 | 0.. | 0x80
PLK_HD_CALL void keccak256_padded(const uint64_t *m, uint64_t *out) {
    uint64_t a[25];
    a[0] = m[0]; a[1] = m[1]; a[2] = m[2]; a[3] = m[3]; a[4] = m[4]; a[5] = m[5]; a[6] = m[6]; a[7] = m[7]; a[8] = m[8];
    a[9] = m[9]; a[10] = m[10]; a[11] = m[11]; a[12] = m[12]; a[13] = m[13]; a[14] = m[14]; a[15] = m[15]; a[16] = m[16];
    a[17] = 0; a[18] = 0; a[19] = 0; a[20] = 0; a[21] = 0; a[22] = 0; a[23] = 0; a[24] = 0;
    keccak_f1600(a);
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
}

// Keccak-256 (Ethereum padding) of a message of len <= 135 bytes given as little-endian lanes, bytes from len on zero; out = the digest's
// four lanes (its 32 bytes read little-endian).  The transcript below does not come through here: its padding sits at fixed places.
PLK_HD void keccak256_one_block(const uint64_t m[17], uint32_t len, uint64_t out[4]) {
    uint64_t p[17];
    for (int i = 0; i < 17; i++) p[i] = m[i];
    p[len >> 3] ^= (uint64_t)0x01 << (8 * (len & 7));
    p[16] ^= (uint64_t)0x80 << 56;
    keccak256_padded(p, out);
}

// ---------------------------------------------------------------------------------------------- RollingKeccakTranscript (keccak.h RollingKeccak)
// s[0..3] / s[4..7]: state_0 / state_1 as the lanes of their digests.  A message is  00 00 00 dom | state_0 | state_1 | tail: everything
// behind the four-byte domain tag sits half a lane off, so lane k of the block is the upper half of word k - 1 and the lower half of word k.
struct RollingKeccakDev {
    uint64_t s[8];
    uint32_t counter;
};

PLK_HD void rk_init(RollingKeccakDev &t) { for (int i = 0; i < 8; i++) t.s[i] = 0; t.counter = 0; }

// absorb_word of the 32 big-endian bytes of c, given as canonical little-endian 32-bit limbs
PLK_HD void rk_absorb_canonical(RollingKeccakDev &t, const uint32_t c[8]) {
    uint64_t m[17], n[8];
    const uint64_t w0 = __builtin_bswap64((uint64_t)c[6] | ((uint64_t)c[7] << 32)), w1 = __builtin_bswap64((uint64_t)c[4] | ((uint64_t)c[5] << 32)),
                   w2 = __builtin_bswap64((uint64_t)c[2] | ((uint64_t)c[3] << 32)), w3 = __builtin_bswap64((uint64_t)c[0] | ((uint64_t)c[1] << 32));
    m[1] = (t.s[0] >> 32) | (t.s[1] << 32); m[2] = (t.s[1] >> 32) | (t.s[2] << 32); m[3] = (t.s[2] >> 32) | (t.s[3] << 32);
    m[4] = (t.s[3] >> 32) | (t.s[4] << 32); m[5] = (t.s[4] >> 32) | (t.s[5] << 32); m[6] = (t.s[5] >> 32) | (t.s[6] << 32);
    m[7] = (t.s[6] >> 32) | (t.s[7] << 32); m[8] = (t.s[7] >> 32) | (w0 << 32); m[9] = (w0 >> 32) | (w1 << 32);
    m[10] = (w1 >> 32) | (w2 << 32); m[11] = (w2 >> 32) | (w3 << 32);
    m[12] = (w3 >> 32) | ((uint64_t)0x01 << 32);                     // byte 100: the first padding byte
    m[13] = 0; m[14] = 0; m[15] = 0; m[16] = (uint64_t)0x80 << 56;
#pragma unroll 1
    for (uint32_t dom = 0; dom < 2; dom++) {                         // state_0' = H(0 | ..), state_1' = H(1 | ..), both over the OLD state
        m[0] = ((uint64_t)dom << 24) | (t.s[0] << 32);
        keccak256_padded(m, n + 4 * dom);
    }
    for (int i = 0; i < 8; i++) t.s[i] = n[i];
}

PLK_HD void rk_absorb_fr(RollingKeccakDev &t, const Fr &v) { const Fr c = to_canonical_call(v); rk_absorb_canonical(t, c.l); }
PLK_HD void rk_absorb_g1(RollingKeccakDev &t, const G1Affine &p) {   // infinity is (0, 0) in memory and is absorbed as (0, 0)
    Fq o = Fq::zero(); o.l[0] = 1;
    const Fq cx = ECM(p.x, o), cy = ECM(p.y, o);
    rk_absorb_canonical(t, cx.l);
    rk_absorb_canonical(t, cy.l);
}

// H(2 | state_0 | state_1 | counter) with the top three bits cleared, as a Montgomery residue (< 2^253 < r: always canonical)
PLK_HD Fr rk_challenge(RollingKeccakDev &t) {
    uint64_t m[17], q[4];
    m[0] = ((uint64_t)2 << 24) | (t.s[0] << 32);
    m[1] = (t.s[0] >> 32) | (t.s[1] << 32); m[2] = (t.s[1] >> 32) | (t.s[2] << 32); m[3] = (t.s[2] >> 32) | (t.s[3] << 32);
    m[4] = (t.s[3] >> 32) | (t.s[4] << 32); m[5] = (t.s[4] >> 32) | (t.s[5] << 32); m[6] = (t.s[5] >> 32) | (t.s[6] << 32);
    m[7] = (t.s[6] >> 32) | (t.s[7] << 32);
    m[8] = (t.s[7] >> 32) | ((uint64_t)__builtin_bswap32(t.counter) << 32);
    m[9] = 0x01;                                                     // byte 72
    m[10] = 0; m[11] = 0; m[12] = 0; m[13] = 0; m[14] = 0; m[15] = 0; m[16] = (uint64_t)0x80 << 56;
    t.counter++;
    keccak256_padded(m, q);
    Fr c;                                                            // the digest read as a big-endian number: byte 0 is the low byte of lane 0
    c.l[7] = __builtin_bswap32((uint32_t)q[0]) & 0x1fffffffu; c.l[6] = __builtin_bswap32((uint32_t)(q[0] >> 32));
    c.l[5] = __builtin_bswap32((uint32_t)q[1]); c.l[4] = __builtin_bswap32((uint32_t)(q[1] >> 32));
    c.l[3] = __builtin_bswap32((uint32_t)q[2]); c.l[2] = __builtin_bswap32((uint32_t)(q[2] >> 32));
    c.l[1] = __builtin_bswap32((uint32_t)q[3]); c.l[0] = __builtin_bswap32((uint32_t)(q[3] >> 32));
    return FRM(c, Fr::r2());
}

// ---------------------------------------------------------------------------------------------- the byte parser (verify.cpp Reader, parse_proof)
// Proofs may start at any byte address: everything is read a byte at a time.
PLK_HD uint64_t front_be64(const uint8_t *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[i]; return v; }

// 32 big-endian bytes -> canonical little-endian limbs; false when the value is >= the modulus
template <class PR>
PLK_HD bool front_be256(const uint8_t *p, Fp<PR> &c) {
    for (int k = 0; k < 8; k++) c.l[7 - k] = ((uint32_t)p[4 * k] << 24) | ((uint32_t)p[4 * k + 1] << 16) | ((uint32_t)p[4 * k + 2] << 8) | (uint32_t)p[4 * k + 3];
    uint64_t br = 0;
    for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)c.l[i] - PR::P[i] - br; br = (d >> 32) & 1; }
    return br != 0;                                                  // a borrow: below the modulus
}

struct FrontReader {
    const uint8_t *p;
    uint64_t left;
};

PLK_HD bool front_u64(FrontReader &r, uint64_t &v) {
    if (r.left < 8) return false;
    v = front_be64(r.p);
    r.p += 8; r.left -= 8;
    return true;
}
// Reader::vec's head: the count, which must be `expect` (0 = any) and must fit into the bytes that are left
PLK_HD bool front_count(FrontReader &r, uint64_t expect, uint64_t item, uint64_t &n) {
    if (!front_u64(r, n)) return false;
    return !((expect && n != expect) || n > r.left / item);
}
PLK_HD_CALL bool front_fr(FrontReader &r, Fr &v) {
    if (r.left < 32) return false;
    Fr c;
    if (!front_be256(r.p, c)) return false;                          // fr >= r
    v = FRM(c, Fr::r2());
    r.p += 32; r.left -= 32;
    return true;
}
// g1_from_bytes and on_curve
PLK_HD_CALL bool front_g1(FrontReader &r, G1Affine &a) {
    if (r.left < 64) return false;
    const uint8_t *in = r.p;
    if (in[0] & 0x40) {                                              // infinity: the flag alone, then zeros
        if (in[0] != 0x40) return false;
        uint32_t any = 0;
        for (int i = 1; i < 64; i++) any |= in[i];
        if (any) return false;
        a.x = Fq::zero(); a.y = Fq::zero();
    } else {
        if (in[0] & 0x80) return false;                              // compression flag on an uncompressed encoding
        Fq cx, cy;
        if (!front_be256(in, cx) || !front_be256(in + 32, cy)) return false;      // fq >= q
        if (cx.is_zero() && cy.is_zero()) return false;              // (0, 0) unflagged: not on the curve
        a.x = ECM(cx, Fq::r2()); a.y = ECM(cy, Fq::r2());
        if (!(ECM(a.y, a.y) == add(ECM(ECM(a.x, a.x), a.x), fq_from_u64_call(3)))) return false;
    }
    r.p += 64; r.left -= 64;
    return true;
}

constexpr int FRONT_PTS = 11;                                        // wires 0..3, grand product 4, quotient 5..8, W_z 9, W_zw 10 (terms 11..21)
constexpr int FRONT_TERMS = 25;

struct FrontProof {
    uint64_t n, num_inputs;
    const uint8_t *inputs;                                           // num_inputs scalars of 32 bytes, each below r
    G1Affine pts[FRONT_PTS];
    Fr wz[4], wzw, z_zw, t_z, r_z, sz[3];
};

// parse_proof over [begin, end): false = malformed.  Never reads outside [begin, end), whatever the counts in the proof say: every read is
// preceded by a comparison with the bytes that are left.
PLK_HD bool front_parse(const uint8_t *begin, const uint8_t *end, FrontProof &P) {
    FrontReader r{begin, (uint64_t)(end - begin)};
    uint64_t n;
    if (!front_u64(r, P.n)) return false;
    if (!front_count(r, 0, 32, P.num_inputs)) return false;
    P.inputs = r.p;
#pragma unroll 1
    for (uint64_t i = 0; i < P.num_inputs; i++) { Fr c; if (!front_be256(r.p, c)) return false; r.p += 32; r.left -= 32; }
    if (!front_count(r, 4, 64, n)) return false;
#pragma unroll 1
    for (int j = 0; j < 4; j++) if (!front_g1(r, P.pts[j])) return false;
    if (!front_g1(r, P.pts[4])) return false;
    if (!front_count(r, 4, 64, n)) return false;
#pragma unroll 1
    for (int j = 0; j < 4; j++) if (!front_g1(r, P.pts[5 + j])) return false;
    if (!front_count(r, 4, 32, n)) return false;
#pragma unroll 1
    for (int j = 0; j < 4; j++) if (!front_fr(r, P.wz[j])) return false;
    if (!front_count(r, 1, 32, n)) return false;
    if (!front_fr(r, P.wzw)) return false;
    if (!front_fr(r, P.z_zw) || !front_fr(r, P.t_z) || !front_fr(r, P.r_z)) return false;
    if (!front_count(r, 3, 32, n)) return false;
#pragma unroll 1
    for (int j = 0; j < 3; j++) if (!front_fr(r, P.sz[j])) return false;
    if (!front_g1(r, P.pts[9]) || !front_g1(r, P.pts[10])) return false;
    return r.left == 0;
}

// ---------------------------------------------------------------------------------------------- flatten_keccak (verify.cpp:199)
PLK_HD_CALL Fr fr_inv_call(const Fr &a) {                                 // Fermat, as HFr::inv; inv(0) = 0
    Fr acc = Fr::one(), base = a;
#pragma unroll 1
    for (int i = 0; i < 256; i++) {
        uint32_t e = FrParams::P[i >> 5];
        if ((i >> 5) == 0) e -= 2;
        if ((e >> (i & 31)) & 1) acc = FRM(acc, base);
        base = FRM(base, base);
    }
    return acc;
}

constexpr uint32_t FRONT_MALFORMED = 2, FRONT_INVALID = 0, FRONT_GOES_ON = 1;

// state 2 = malformed, 0 = settled invalid, 1 = goes on to the group arithmetic; pts[11] and sc[25] are written for state 1 only.
// The early returns keep flatten_keccak's order: malformed, size / input count / strict rule, z^N == 1, the equation at z.
PLK_HD uint32_t flatten_front(const FrontVk &vk, const uint8_t *begin, const uint8_t *end, G1Affine *pts, Fr *sc) {
    FrontProof P;
    if (!front_parse(begin, end, P)) return FRONT_MALFORMED;
    const uint64_t N = vk.n + 1;
    if (N < 2 || (N & (N - 1)) || N > (1ull << 28)) return FRONT_INVALID;
    uint32_t log_n = 0; while ((1ull << log_n) < N) log_n++;
    if ((vk.flags & 1u) && vk.num_inputs < 1) return FRONT_INVALID;  // PLK_VERIFY_STRICT_INPUTS
    if (P.n != vk.n || P.num_inputs != vk.num_inputs) return FRONT_INVALID;
    const Fr om = vk.omega, one = Fr::one();
    RollingKeccakDev tr; rk_init(tr);
#pragma unroll 1
    for (uint64_t i = 0; i < P.num_inputs; i++) { Fr c; (void)front_be256(P.inputs + 32 * i, c); rk_absorb_canonical(tr, c.l); }
#pragma unroll 1
    for (int j = 0; j < 4; j++) rk_absorb_g1(tr, P.pts[j]);
    const Fr beta = rk_challenge(tr), gamma = rk_challenge(tr);
    rk_absorb_g1(tr, P.pts[4]);
    const Fr alpha = rk_challenge(tr);
#pragma unroll 1
    for (int j = 0; j < 4; j++) rk_absorb_g1(tr, P.pts[5 + j]);
    const Fr z = rk_challenge(tr);
    Fr zN = z;
#pragma unroll 1
    for (uint32_t i = 0; i < log_n; i++) zN = FRM(zN, zN);
    if (zN == one) return FRONT_INVALID;
    // L_i(z) = w^i (z^N - 1) / (N (z - w^i)) for the public-input rows; L_0(z) is needed whatever the number of inputs
    const Fr zn1 = sub(zN, one);
    Fr rhs = P.r_z, lag0 = Fr::zero();
    {
        Fr wi = one; const Fr nf = fr_from_u64_call(N);
        const uint64_t rows = vk.num_inputs ? vk.num_inputs : 1;
#pragma unroll 1
        for (uint64_t i = 0; i < rows; i++) {
            const Fr li = FRM(FRM(wi, zn1), fr_inv_call(FRM(nf, sub(z, wi))));
            if (i == 0) lag0 = li;
            if (i < vk.num_inputs) { Fr c; (void)front_be256(P.inputs + 32 * i, c); rhs = add(rhs, FRM(li, FRM(c, Fr::r2()))); }
            wi = FRM(wi, om);
        }
    }
    const Fr l0aa = FRM(FRM(lag0, alpha), alpha);
    {   // verify_at_z: t(z) (z^N - 1) == r(z) + PI(z) - alpha z(zw) prod_j(..) (gamma + d) - alpha^2 L_0(z)
        const Fr lhs = FRM(zn1, P.t_z);
        Fr zpart = P.z_zw;
#pragma unroll 1
        for (int j = 0; j < 3; j++) zpart = FRM(zpart, add(add(FRM(P.sz[j], beta), gamma), P.wz[j]));
        zpart = FRM(FRM(zpart, add(gamma, P.wz[3])), alpha);
        rhs = sub(sub(rhs, zpart), l0aa);
        if (!(lhs == rhs)) return FRONT_INVALID;
    }
#pragma unroll 1
    for (int j = 0; j < 4; j++) rk_absorb_fr(tr, P.wz[j]);
    rk_absorb_fr(tr, P.wzw);
#pragma unroll 1
    for (int j = 0; j < 3; j++) rk_absorb_fr(tr, P.sz[j]);
    rk_absorb_fr(tr, P.t_z); rk_absorb_fr(tr, P.r_z); rk_absorb_fr(tr, P.z_zw);
    const Fr v = rk_challenge(tr);
    rk_absorb_g1(tr, P.pts[9]); rk_absorb_g1(tr, P.pts[10]);
    const Fr u = rk_challenge(tr);

    for (int j = 0; j < FRONT_PTS; j++) pts[j] = P.pts[j];
    // d = v (q_const + sum wz_j q_j + wz_0 wz_1 q_m + wire_zw q_next + gz Z - last sigma_3) + gzw Z
    for (int j = 0; j < 4; j++) sc[j] = FRM(v, P.wz[j]);
    sc[4] = FRM(FRM(v, P.wz[0]), P.wz[1]);
    sc[5] = v;
    sc[6] = FRM(v, P.wzw);
    Fr gz = add(add(FRM(z, beta), P.wz[0]), gamma);
#pragma unroll 1
    for (int j = 0; j < 3; j++) gz = FRM(gz, add(add(FRM(FRM(z, vk.non_residues[j]), beta), gamma), P.wz[j + 1]));
    gz = add(FRM(gz, alpha), l0aa);
    Fr v9 = one;
#pragma unroll 1
    for (int i = 0; i < 9; i++) v9 = FRM(v9, v);
    Fr last = one;
#pragma unroll 1
    for (int j = 0; j < 3; j++) last = FRM(last, add(add(FRM(beta, P.sz[j]), gamma), P.wz[j]));
    last = FRM(FRM(FRM(last, beta), P.z_zw), alpha);
    sc[10] = neg(FRM(v, last));
    sc[15] = add(FRM(v, gz), FRM(v9, u));
    // agg = t_0 + sum zN^k t_k + d + sum ch wires + sum ch sigma + ch u wires_3 - val G
    Fr zk = one;
    sc[16] = one;
    for (int k = 1; k < 4; k++) { zk = FRM(zk, zN); sc[16 + k] = zk; }
    Fr ch = v;
    for (int j = 0; j < 3; j++) { ch = FRM(ch, v); sc[11 + j] = ch; }
    ch = FRM(ch, v);
    const Fr ch14 = ch;
    for (int j = 0; j < 3; j++) { ch = FRM(ch, v); sc[7 + j] = ch; }
    ch = FRM(ch, v); ch = FRM(ch, v);
    sc[14] = add(ch14, FRM(ch, u));
    ch = v;
    Fr val = add(P.t_z, FRM(P.r_z, ch));
#pragma unroll 1
    for (int j = 0; j < 4; j++) { ch = FRM(ch, v); val = add(val, FRM(P.wz[j], ch)); }
#pragma unroll 1
    for (int j = 0; j < 3; j++) { ch = FRM(ch, v); val = add(val, FRM(P.sz[j], ch)); }
    ch = FRM(ch, v); val = add(val, FRM(FRM(P.z_zw, ch), u));
    ch = FRM(ch, v); val = add(val, FRM(FRM(P.wzw, ch), u));
    sc[22] = neg(val);
    // pg = agg + z W_z + z omega u W_zw ;  px = -(W_z + u W_zw)
    sc[20] = z; sc[21] = FRM(FRM(z, om), u);
    sc[23] = neg(one); sc[24] = neg(u);
    return FRONT_GOES_ON;
}

}  // namespace plk
