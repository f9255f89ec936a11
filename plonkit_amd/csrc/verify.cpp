// PLONK verifier on the host: bellman_ce::plonk::better_cs::verifier::verify as plonkit calls it
// (reference call site src/plonk.rs:189-210, CLI src/bin/main.rs:425-437); the algorithm is the one the
// reference's Solidity template spells out (contrib/template.sol:445-494 verify_initial, 496-586
// verify_at_z, 588-689 reconstruct_d, 691-758 verify_commitments) over the file formats of SURVEY.md A.1.
// The transcript is the built-in Keccak one (`-t keccak`) or the caller's table (transcript_ops.h); CPU code in the reference too.
#include <cstdlib>
#include "../../include/plonkit_amd.h"
#include "keccak.h"
#include "pairing.h"
#include "verify_many.h"
#include "transcript_ops.h"
#include <string>
#include <vector>

namespace plk { void set_error(const std::string &msg); }
#define PLK_API extern "C" __attribute__((visibility("default")))
using namespace plk;
using namespace plk::host;

namespace {

template <class T> constexpr uint64_t sizeof_item() { return 64; }              // G1 (uncompressed)
template <> constexpr uint64_t sizeof_item<HFr>() { return 32; }

struct Reader {
    const uint8_t *p; uint64_t left; bool ok = true;
    uint64_t u64() {
        if (left < 8) { ok = false; return 0; }
        uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[i];
        p += 8; left -= 8; return v;
    }
    HFr fr() {
        HFr v = HFr::zero();
        if (left < 32) { ok = false; return v; }
        if (!HFr::from_be_bytes(p, &v)) ok = false;
        p += 32; left -= 32; return v;
    }
    HAffine g1() {
        HAffine a; a.x = HFq::zero(); a.y = HFq::zero();
        if (left < 64) { ok = false; return a; }
        if (!g1_from_bytes(p, &a) || !on_curve(a)) ok = false;
        p += 64; left -= 64; return a;
    }
    G2Affine g2() {
        G2Affine a; a.inf = true; a.x = Fq2::zero(); a.y = Fq2::zero();
        if (left < 128) { ok = false; return a; }
        if (!g2_from_bytes(p, &a)) ok = false;
        p += 128; left -= 128; return a;
    }
    template <class T, class Fn> bool vec(std::vector<T> &out, uint64_t expect, Fn rd) {
        uint64_t n = u64();
        if (!ok || (expect && n != expect) || n > left / sizeof_item<T>()) { ok = false; return false; }   // bounded by the bytes that are left
        for (uint64_t i = 0; i < n && ok; i++) out.push_back(rd());
        return ok;
    }
};

struct Vk {
    uint64_t n, num_inputs;
    std::vector<HAffine> selectors, next_step, sigma;
    std::vector<HFr> non_residues;
    G2Affine g2[2];
};
struct ProofData {
    uint64_t n;
    std::vector<HFr> inputs, wire_z, wire_zw, sigma_z;
    std::vector<HAffine> wires, quotient;
    HAffine grand_product, open_z, open_zw;
    HFr z_zw, t_z, r_z;
};

bool parse_vk(const uint8_t *b, uint64_t len, Vk *vk) {
    Reader r{b, len};
    vk->n = r.u64(); vk->num_inputs = r.u64();
    r.vec(vk->selectors, 6, [&] { return r.g1(); });
    r.vec(vk->next_step, 1, [&] { return r.g1(); });
    r.vec(vk->sigma, 4, [&] { return r.g1(); });
    r.vec(vk->non_residues, 3, [&] { return r.fr(); });
    vk->g2[0] = r.g2(); vk->g2[1] = r.g2();
    return r.ok && r.left == 0;
}
bool parse_proof(const uint8_t *b, uint64_t len, ProofData *p) {
    Reader r{b, len};
    p->n = r.u64();
    r.vec(p->inputs, 0, [&] { return r.fr(); });
    r.vec(p->wires, 4, [&] { return r.g1(); });
    p->grand_product = r.g1();
    r.vec(p->quotient, 4, [&] { return r.g1(); });
    r.vec(p->wire_z, 4, [&] { return r.fr(); });
    r.vec(p->wire_zw, 1, [&] { return r.fr(); });
    p->z_zw = r.fr(); p->t_z = r.fr(); p->r_z = r.fr();
    r.vec(p->sigma_z, 3, [&] { return r.fr(); });
    p->open_z = r.g1(); p->open_zw = r.g1();
    return r.ok && r.left == 0;
}

HFr omega_of(uint32_t log_n) {                                // omega_{2^28} = 7^((r-1)/2^28), SURVEY.md A.2
    const uint64_t c[4] = {0xd34f1ed960c37c9cULL, 0x3215cf6dd39329c8ULL, 0x98865ea93dd31f74ULL, 0x03ddb9f5166d18b7ULL};
    HFr w = HFr::from_canonical(c);
    for (uint32_t i = log_n; i < 28; i++) w = w.sqr();
    return w;
}

HJac smul(const HAffine &p, const HFr &k) { uint64_t c[4]; k.to_canonical(c); return jac_mul(jac_from_affine(p), c); }
HJac smulj(const HJac &p, const HFr &k) { uint64_t c[4]; k.to_canonical(c); return jac_mul(p, c); }

// Tr: KeccakTranscript (ops unused: the code of the Keccak-only verifier) or ProofTranscript over the caller's table.  *tr_rc / *tr_msg: a
// failure of the caller's transcript (the result is false then and means nothing)
template <class Tr> bool verify_keccak(const Vk &vk, const ProofData &P, bool strict_inputs, const plk_transcript_ops *ops = nullptr, int32_t *tr_rc = nullptr,
                   std::string *tr_msg = nullptr) {
    const uint64_t N = vk.n + 1;
    if (N < 2 || (N & (N - 1)) || N > (1ull << 28)) return false;
    uint32_t log_n = 0; while ((1ull << log_n) < N) log_n++;
    // PLK_VERIFY_STRICT_INPUTS: the Solidity verifier's `require(vk.num_inputs >= 1)` (contrib/template.sol:697) for deployments
    // whose proofs end up on chain; off by default, see below
    if (strict_inputs && vk.num_inputs < 1) return false;
    // contrib/template.sol:697 additionally requires num_inputs >= 1 — a restriction of the SOLIDITY verifier only.  `plonkit
    // verify` calls bellman's Rust verifier::verify (src/plonk.rs:196), which walks proof.input_values with no such
    // requirement [recollection; unpinned: no fixture has zero inputs], and a circom circuit without public signals is
    // legal (num_inputs = 1 = wire ONE only, src/reader.rs:197, src/circom_circuit.rs:78): zero inputs are accepted here.
    if (P.n != vk.n || P.inputs.size() != vk.num_inputs) return false;
    const HFr om = omega_of(log_n), one = HFr::one();
    Tr tr(ops, "plk_verify");
    TranscriptOutcome<Tr> tr_out{tr, tr_rc, tr_msg};
    (void)tr_out;
    for (const HFr &x : P.inputs) tr.absorb_fr(x);
    for (const HAffine &c : P.wires) tr.absorb_g1(c);
    const HFr beta = tr.challenge(), gamma = tr.challenge();
    if (tr.status() != PLK_OK) return false;
    tr.absorb_g1(P.grand_product);
    const HFr alpha = tr.challenge();
    if (tr.status() != PLK_OK) return false;
    for (const HAffine &c : P.quotient) tr.absorb_g1(c);
    const HFr z = tr.challenge();
    if (tr.status() != PLK_OK) return false;
    HFr zN = z; for (uint32_t i = 0; i < log_n; i++) zN = zN.sqr();
    if (zN == one) return false;
    // L_i(z) = w^i (z^N - 1) / (N (z - w^i)) for the public-input rows
    std::vector<HFr> lag(vk.num_inputs ? vk.num_inputs : 1);          // L_0(z) is needed whatever the number of inputs
    { HFr wi = one; const HFr nf = HFr::from_u64(N);
      for (uint64_t i = 0; i < lag.size(); i++) { lag[i] = wi * (zN - one) * (nf * (z - wi)).inv(); wi = wi * om; } }
    const std::vector<HFr> &wz = P.wire_z, &sz = P.sigma_z;
    // verify_at_z: t(z) (z^N - 1) == r(z) + PI(z) - alpha z(zw) prod_j(..) (gamma + d) - alpha^2 L_0(z)
    {
        const HFr lhs = (zN - one) * P.t_z;
        HFr rhs = P.r_z;
        for (uint64_t i = 0; i < vk.num_inputs; i++) rhs = rhs + lag[i] * P.inputs[i];
        HFr zpart = P.z_zw;
        for (int j = 0; j < 3; j++) zpart = zpart * (sz[j] * beta + gamma + wz[j]);
        zpart = zpart * (gamma + wz[3]) * alpha;
        rhs = rhs - zpart - lag[0] * alpha * alpha;
        if (!(lhs == rhs)) return false;
    }
    for (const HFr &x : wz) tr.absorb_fr(x);
    for (const HFr &x : P.wire_zw) tr.absorb_fr(x);
    for (const HFr &x : sz) tr.absorb_fr(x);
    tr.absorb_fr(P.t_z); tr.absorb_fr(P.r_z); tr.absorb_fr(P.z_zw);
    const HFr v = tr.challenge();
    if (tr.status() != PLK_OK) return false;
    tr.absorb_g1(P.open_z); tr.absorb_g1(P.open_zw);
    const HFr u = tr.challenge();
    if (tr.status() != PLK_OK) return false;

    // reconstruct_d: the commitment of the linearisation polynomial
    HJac d = jac_from_affine(vk.selectors[5]);
    for (int j = 0; j < 4; j++) d = jac_add(d, smul(vk.selectors[j], wz[j]));
    d = jac_add(d, smul(vk.selectors[4], wz[0] * wz[1]));
    d = jac_add(d, smul(vk.next_step[0], P.wire_zw[0]));
    HFr gz = z * beta + wz[0] + gamma;
    for (int j = 0; j < 3; j++) gz = gz * (z * vk.non_residues[j] * beta + gamma + wz[j + 1]);
    gz = gz * alpha + lag[0] * alpha * alpha;
    HFr v9 = one; for (int i = 0; i < 9; i++) v9 = v9 * v;      // v^(1 + 1 + 4 + 4 - 1)
    const HFr gzw = v9 * u;
    HFr last = one;
    for (int j = 0; j < 3; j++) last = last * (beta * sz[j] + gamma + wz[j]);
    last = last * beta * P.z_zw * alpha;
    HJac t = jac_add(smul(P.grand_product, gz), jac_neg(smul(vk.sigma[3], last)));
    d = smulj(jac_add(d, t), v);
    d = jac_add(d, smul(P.grand_product, gzw));

    // verify_commitments: aggregate the openings at z and z*omega
    HJac agg = jac_from_affine(P.quotient[0]);
    { HFr tf = one; for (int k = 1; k < 4; k++) { tf = tf * zN; agg = jac_add(agg, smul(P.quotient[k], tf)); } }
    HFr ch = v;
    agg = jac_add(agg, d);
    for (const HAffine &c : P.wires) { ch = ch * v; agg = jac_add(agg, smul(c, ch)); }
    for (int j = 0; j < 3; j++) { ch = ch * v; agg = jac_add(agg, smul(vk.sigma[j], ch)); }
    ch = ch * v; ch = ch * v;
    agg = jac_add(agg, smul(P.wires[3], ch * u));
    ch = v;
    HFr val = P.t_z + P.r_z * ch;
    for (const HFr &x : wz) { ch = ch * v; val = val + x * ch; }
    for (const HFr &x : sz) { ch = ch * v; val = val + x * ch; }
    ch = ch * v; val = val + P.z_zw * ch * u;
    ch = ch * v; val = val + P.wire_zw[0] * ch * u;
    HAffine G; G.x = HFq::from_u64(1); G.y = HFq::from_u64(2);
    agg = jac_add(agg, jac_neg(smul(G, val)));
    HJac pg = jac_add(agg, smul(P.open_z, z));
    pg = jac_add(pg, smul(P.open_zw, z * om * u));
    HJac px = jac_neg(jac_add(smul(P.open_zw, u), jac_from_affine(P.open_z)));
    // e(pg, g2[0]) * e(px, g2[1]) == 1
    const HAffine g1s[2] = {jac_to_affine(pg), jac_to_affine(px)};
    return pairing_product_is_one(g1s, vk.g2, 2);
}

// The same verifier up to the pairing, FLATTENED: every nested expression of verify_keccak above (d, agg, val) collapsed into one scalar per
// distinct point, so that pg = sum_{k<23} s_k P_k and px = s_23 P_23 + s_24 P_24 can be formed by independent scalar multiplications
// (verify_many.hip).  Returns false where verify_keccak returns false before any group arithmetic.  verify_keccak keeps its own arithmetic;
// tests/test_verify_terms_host.py pins the two against each other.
template <class Tr> bool flatten_keccak(const Vk &vk, const ProofData &P, bool strict_inputs, HAffine pts[VERIFY_TERMS], HFr sc[VERIFY_TERMS],
                    const plk_transcript_ops *ops = nullptr, int32_t *tr_rc = nullptr, std::string *tr_msg = nullptr) {
    const uint64_t N = vk.n + 1;
    if (N < 2 || (N & (N - 1)) || N > (1ull << 28)) return false;
    uint32_t log_n = 0; while ((1ull << log_n) < N) log_n++;
    if (strict_inputs && vk.num_inputs < 1) return false;
    if (P.n != vk.n || P.inputs.size() != vk.num_inputs) return false;
    const HFr om = omega_of(log_n), one = HFr::one();
    Tr tr(ops, "plk_verify");
    TranscriptOutcome<Tr> tr_out{tr, tr_rc, tr_msg};
    (void)tr_out;
    for (const HFr &x : P.inputs) tr.absorb_fr(x);
    for (const HAffine &c : P.wires) tr.absorb_g1(c);
    const HFr beta = tr.challenge(), gamma = tr.challenge();
    if (tr.status() != PLK_OK) return false;
    tr.absorb_g1(P.grand_product);
    const HFr alpha = tr.challenge();
    if (tr.status() != PLK_OK) return false;
    for (const HAffine &c : P.quotient) tr.absorb_g1(c);
    const HFr z = tr.challenge();
    if (tr.status() != PLK_OK) return false;
    HFr zN = z; for (uint32_t i = 0; i < log_n; i++) zN = zN.sqr();
    if (zN == one) return false;
    std::vector<HFr> lag(vk.num_inputs ? vk.num_inputs : 1);
    { HFr wi = one; const HFr nf = HFr::from_u64(N);
      for (uint64_t i = 0; i < lag.size(); i++) { lag[i] = wi * (zN - one) * (nf * (z - wi)).inv(); wi = wi * om; } }
    const std::vector<HFr> &wz = P.wire_z, &sz = P.sigma_z;
    {
        const HFr lhs = (zN - one) * P.t_z;
        HFr rhs = P.r_z;
        for (uint64_t i = 0; i < vk.num_inputs; i++) rhs = rhs + lag[i] * P.inputs[i];
        HFr zpart = P.z_zw;
        for (int j = 0; j < 3; j++) zpart = zpart * (sz[j] * beta + gamma + wz[j]);
        zpart = zpart * (gamma + wz[3]) * alpha;
        rhs = rhs - zpart - lag[0] * alpha * alpha;
        if (!(lhs == rhs)) return false;
    }
    for (const HFr &x : wz) tr.absorb_fr(x);
    for (const HFr &x : P.wire_zw) tr.absorb_fr(x);
    for (const HFr &x : sz) tr.absorb_fr(x);
    tr.absorb_fr(P.t_z); tr.absorb_fr(P.r_z); tr.absorb_fr(P.z_zw);
    const HFr v = tr.challenge();
    if (tr.status() != PLK_OK) return false;
    tr.absorb_g1(P.open_z); tr.absorb_g1(P.open_zw);
    const HFr u = tr.challenge();
    if (tr.status() != PLK_OK) return false;

    // points: selectors 0..5, next_step 6, sigma 7..10 | wires 11..14, grand product 15, quotient 16..19, W_z 20, W_zw 21 | G 22 | W_z 23, W_zw 24
    for (int j = 0; j < 6; j++) pts[j] = vk.selectors[j];
    pts[6] = vk.next_step[0];
    for (int j = 0; j < 4; j++) pts[7 + j] = vk.sigma[j];
    for (int j = 0; j < 4; j++) pts[11 + j] = P.wires[j];
    pts[15] = P.grand_product;
    for (int j = 0; j < 4; j++) pts[16 + j] = P.quotient[j];
    pts[20] = P.open_z; pts[21] = P.open_zw;
    pts[22].x = HFq::from_u64(1); pts[22].y = HFq::from_u64(2);
    pts[23] = P.open_z; pts[24] = P.open_zw;

    // d = v (q_const + sum wz_j q_j + wz_0 wz_1 q_m + wire_zw q_next + gz Z - last sigma_3) + gzw Z
    for (int j = 0; j < 4; j++) sc[j] = v * wz[j];
    sc[4] = v * wz[0] * wz[1];
    sc[5] = v;
    sc[6] = v * P.wire_zw[0];
    HFr gz = z * beta + wz[0] + gamma;
    for (int j = 0; j < 3; j++) gz = gz * (z * vk.non_residues[j] * beta + gamma + wz[j + 1]);
    gz = gz * alpha + lag[0] * alpha * alpha;
    HFr v9 = one; for (int i = 0; i < 9; i++) v9 = v9 * v;
    HFr last = one;
    for (int j = 0; j < 3; j++) last = last * (beta * sz[j] + gamma + wz[j]);
    last = last * beta * P.z_zw * alpha;
    sc[10] = -(v * last);
    sc[15] = v * gz + v9 * u;
    // agg = t_0 + sum zN^k t_k + d + sum ch wires + sum ch sigma + ch u wires_3 - val G
    sc[16] = one;
    for (int k = 1; k < 4; k++) sc[16 + k] = sc[16 + k - 1] * zN;
    HFr ch = v;
    for (int j = 0; j < 4; j++) { ch = ch * v; sc[11 + j] = ch; }
    for (int j = 0; j < 3; j++) { ch = ch * v; sc[7 + j] = ch; }
    ch = ch * v; ch = ch * v;
    sc[14] = sc[14] + ch * u;
    ch = v;
    HFr val = P.t_z + P.r_z * ch;
    for (const HFr &x : wz) { ch = ch * v; val = val + x * ch; }
    for (const HFr &x : sz) { ch = ch * v; val = val + x * ch; }
    ch = ch * v; val = val + P.z_zw * ch * u;
    ch = ch * v; val = val + P.wire_zw[0] * ch * u;
    sc[22] = -val;
    // pg = agg + z W_z + z omega u W_zw ;  px = -(W_z + u W_zw)
    sc[20] = z; sc[21] = z * om * u;
    sc[23] = -one; sc[24] = -u;
    return true;
}

}  // namespace

namespace plk {
// ParsedVk is never defined: the handle is this file's Vk under a name other translation units can spell
static const Vk &vk_of(const ParsedVk *v) { return *reinterpret_cast<const Vk *>(v); }
ParsedVk *parsed_vk_new(const uint8_t *vk, uint64_t len) {
    Vk *p = new Vk;
    if (!parse_vk(vk, len, p)) { delete p; return nullptr; }
    return reinterpret_cast<ParsedVk *>(p);
}
void parsed_vk_free(ParsedVk *v) { delete reinterpret_cast<Vk *>(v); }
ParsedVk *parsed_vk_clone(const ParsedVk *v) { return reinterpret_cast<ParsedVk *>(new Vk(vk_of(v))); }
void parsed_vk_points(const ParsedVk *v, plk_g1_affine fixed[VERIFY_FIXED], host::G2Affine g2[2]) {
    const Vk &k = vk_of(v);
    for (int j = 0; j < 6; j++) memcpy(&fixed[j], &k.selectors[j], 64);
    memcpy(&fixed[6], &k.next_step[0], 64);
    for (int j = 0; j < 4; j++) memcpy(&fixed[7 + j], &k.sigma[j], 64);
    HAffine G; G.x = HFq::from_u64(1); G.y = HFq::from_u64(2);
    memcpy(&fixed[11], &G, 64);
    g2[0] = k.g2[0]; g2[1] = k.g2[1];
}
void parsed_vk_front(const ParsedVk *v, uint64_t *n, uint64_t *num_inputs, plk_fr non_residues[3], plk_fr *omega) {
    const Vk &k = vk_of(v);
    *n = k.n; *num_inputs = k.num_inputs;
    for (int j = 0; j < 3; j++) memcpy(&non_residues[j], &k.non_residues[j], 32);
    const uint64_t N = k.n + 1;
    HFr om = HFr::zero();                                             // a size that flatten_keccak refuses has no omega, and none is asked for
    if (!(N < 2 || (N & (N - 1)) || N > (1ull << 28))) { uint32_t log_n = 0; while ((1ull << log_n) < N) log_n++; om = omega_of(log_n); }
    memcpy(omega, &om, 32);
}
int32_t verify_terms_parsed(const ParsedVk *v, const uint8_t *proof, uint64_t len, uint32_t flags, plk_g1_affine points[VERIFY_TERMS],
                            plk_fr scalars[VERIFY_TERMS], int32_t *early, const plk_transcript_ops *ops, std::string *tr_msg) {
    ProofData pr;
    if (!parse_proof(proof, len, &pr)) { set_error("plk_verify: malformed proof"); return PLK_ERR_ARG; }
    HAffine pts[VERIFY_TERMS]; HFr sc[VERIFY_TERMS];
    memset(points, 0, VERIFY_TERMS * sizeof(plk_g1_affine)); memset(scalars, 0, VERIFY_TERMS * sizeof(plk_fr));
    int32_t tr_rc = PLK_OK;
    const bool strict = (flags & PLK_VERIFY_STRICT_INPUTS) != 0;
    *early = (ops ? flatten_keccak<ProofTranscript>(vk_of(v), pr, strict, pts, sc, ops, &tr_rc, tr_msg)
                  : flatten_keccak<KeccakTranscript>(vk_of(v), pr, strict, pts, sc)) ? 1 : 0;
    if (tr_rc != PLK_OK) { *early = 0; return tr_rc; }
    if (*early) for (int k = 0; k < VERIFY_TERMS; k++) { memcpy(&points[k], &pts[k], 64); memcpy(&scalars[k], &sc[k], 32); }
    return PLK_OK;
}
}  // namespace plk

// what plk_verify_with, plk_verify_terms_with and plk_verify_many_with ask of a table before they use it
static int32_t check_ops(const plk_transcript_ops *ops, const char *who) {
    if (!ops) return PLK_OK;
    if (!transcript_ops_complete(ops)) { set_error(std::string(who) + ": the transcript table has a null callback"); return PLK_ERR_ARG; }
    if (ops->flags & ~(uint32_t)PLK_TRANSCRIPT_CONCURRENT) { set_error(std::string(who) + ": unknown flag in the transcript table"); return PLK_ERR_ARG; }
    return PLK_OK;
}

PLK_API int32_t plk_verify_terms_with(const uint8_t *vk_bytes, uint64_t vk_len, const uint8_t *proof_bytes, uint64_t proof_len, uint32_t flags,
                                      const plk_transcript_ops *ops, plk_g1_affine points[25], plk_fr scalars[25], int32_t *early) {
    if (!vk_bytes || !proof_bytes || !points || !scalars || !early) { set_error("plk_verify_terms: null argument"); return PLK_ERR_ARG; }
    if (flags & ~(uint32_t)PLK_VERIFY_STRICT_INPUTS) { set_error("plk_verify_ex: unknown flag"); return PLK_ERR_ARG; }
    if (const int32_t rc = check_ops(ops, "plk_verify_terms_with")) return rc;
    const plk_transcript_ops table = ops ? *ops : plk_transcript_ops{};       // the caller's struct is copied, as plk_ctx_set_transcript copies it
    ParsedVk *v = parsed_vk_new(vk_bytes, vk_len);
    if (!v) { set_error("plk_verify: malformed verification key"); return PLK_ERR_ARG; }
    std::string tr_msg;
    const int32_t rc = verify_terms_parsed(v, proof_bytes, proof_len, flags, points, scalars, early, ops ? &table : nullptr, &tr_msg);
    if (!tr_msg.empty()) set_error(tr_msg);
    parsed_vk_free(v);
    return rc;
}

PLK_API int32_t plk_verify_terms(const uint8_t *vk_bytes, uint64_t vk_len, const uint8_t *proof_bytes, uint64_t proof_len, uint32_t flags,
                                 plk_g1_affine points[25], plk_fr scalars[25], int32_t *early) {
    return plk_verify_terms_with(vk_bytes, vk_len, proof_bytes, proof_len, flags, nullptr, points, scalars, early);
}

PLK_API int32_t plk_verify_with(const uint8_t *vk_bytes, uint64_t vk_len, const uint8_t *proof_bytes, uint64_t proof_len, uint32_t flags,
                                const plk_transcript_ops *ops, int32_t *valid) {
    if (!vk_bytes || !proof_bytes || !valid) { set_error("plk_verify: null argument"); return PLK_ERR_ARG; }
    if (flags & ~(uint32_t)PLK_VERIFY_STRICT_INPUTS) { set_error("plk_verify_ex: unknown flag"); return PLK_ERR_ARG; }
    if (const int32_t rc = check_ops(ops, "plk_verify_with")) return rc;
    const plk_transcript_ops table = ops ? *ops : plk_transcript_ops{};
    Vk vk; ProofData pr;
    if (!parse_vk(vk_bytes, vk_len, &vk)) { set_error("plk_verify: malformed verification key"); return PLK_ERR_ARG; }
    if (!parse_proof(proof_bytes, proof_len, &pr)) { set_error("plk_verify: malformed proof"); return PLK_ERR_ARG; }
    int32_t tr_rc = PLK_OK; std::string tr_msg;
    const bool strict = (flags & PLK_VERIFY_STRICT_INPUTS) != 0;
    const bool ok = ops ? verify_keccak<ProofTranscript>(vk, pr, strict, &table, &tr_rc, &tr_msg) : verify_keccak<KeccakTranscript>(vk, pr, strict);
    if (tr_rc != PLK_OK) { set_error(tr_msg); return tr_rc; }
    *valid = ok ? 1 : 0;
    return PLK_OK;
}

PLK_API int32_t plk_verify_ex(const uint8_t *vk_bytes, uint64_t vk_len, const uint8_t *proof_bytes, uint64_t proof_len, uint32_t flags, int32_t *valid) {
    return plk_verify_with(vk_bytes, vk_len, proof_bytes, proof_len, flags, nullptr, valid);
}

PLK_API int32_t plk_verify(const uint8_t *vk_bytes, uint64_t vk_len, const uint8_t *proof_bytes, uint64_t proof_len, int32_t *valid) {
    const char *e = getenv("PLK_VERIFY_STRICT_INPUTS");               // read per call: a test (or a service) may flip it
    return plk_verify_ex(vk_bytes, vk_len, proof_bytes, proof_len, (e && e[0] && e[0] != '0') ? PLK_VERIFY_STRICT_INPUTS : 0u, valid);
}

PLK_API int32_t plk_pairing_check(const plk_g1_affine *a, const uint8_t *g2_a, const plk_g1_affine *b, const uint8_t *g2_b, int32_t *is_one) {
    if (!a || !b || !g2_a || !g2_b || !is_one) { set_error("plk_pairing_check: null argument"); return PLK_ERR_ARG; }
    HAffine g1s[2]; G2Affine g2s[2];
    memcpy(&g1s[0], a, 64); memcpy(&g1s[1], b, 64);
    if (!on_curve(g1s[0]) || !on_curve(g1s[1])) { set_error("plk_pairing_check: G1 point not on the curve"); return PLK_ERR_ARG; }
    if (!g2_from_bytes(g2_a, &g2s[0]) || !g2_from_bytes(g2_b, &g2s[1])) { set_error("plk_pairing_check: G2 point not on the twist"); return PLK_ERR_ARG; }
    *is_one = pairing_product_is_one(g1s, g2s, 2) ? 1 : 0;
    return PLK_OK;
}
