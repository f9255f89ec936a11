// Many proofs of one verification key, each verified exactly and on its own (plk_vk_load, plk_verify_many, plk_pairing_check_many_dev).
// NO COUNTERPART IN THE REFERENCE, whose plonk::verify (src/plonk.rs:189-210) takes one proof on one host thread; verdict i is what
// plk_verify_ex says about proof i.  There is no random linear combination across proofs and no shared pairing.
//
// Host, per proof, on up to 16 threads: parse, transcript, the scalar checks, and the flattened scalars of verify.cpp (plk_verify_terms).
// plk_verify_many_packed / plk_verify_many_dev / plk_verify_front_dev run that front end on the device instead, from the raw bytes
// (vm_front_kernel, verify_front.hip): every proof of a pass then goes through the kernels below, a proof the front end settled as all-zero
// terms, and vm_settle_kernel writes its verdict from the state byte.
// Device, for the proofs that pass that:
//   vm_mul_kernel      one (proof, term) per lane, 25 terms per proof: the GLV double-and-add of g1_mul_dev.h with four effectively affine
//                      table entries (g1_mul_scalar_iso: 72 KB of LDS per 256 lanes, two workgroups per CU)
//   vm_sum_kernel      one lane per (proof, side): 23 -> 1 and 2 -> 1 on the 29-bit layer, left as XYZZ in the external form
//   vm_affine_kernel   XYZZ -> affine, one inversion per 8 points (as srs_to_affine_kernel); infinity comes out as x = y = 0
//   vm_pairing_kernel  one proof per lane: f <- f^2 l_0 l_1 over the uploaded line table, then the shortened final exponentiation of
//                      fq12_dev.h (which decides the same predicate as pairing.cpp's; the argument is written there)
// A key set (plk_vkset_create, plk_verify_mixed, _packed, _dev) verifies proofs of several keys in one pass, the key taken per proof:
// vm_mul_mixed_kernel and vm_pairing_mixed_kernel are the two kernels above with the key's points and line table looked up per lane
// (vkset_dev.h), vm_front_mixed_kernel (verify_front.hip) likewise; the other kernels serve both.
// Host side, in this order: the kernels; plk_vk and plk_vkset; VmArena (the layout of vm_arena.h); VmKeys, one key or a key set, which holds
// everything that differs between the two; vm_pass, the one order of launches; and one driver per input form (host-parsed proofs, packed
// bytes on the host, bytes on the device), each behind its two extern "C" calls.
#include "ctx.h"
#include "ec_dev.h"
#include "ec29_dev.h"
#include "glv_dev.h"
#include "g1_mul_dev.h"
#include "fq12_dev.h"
#include "pairing_table.h"
#include "verify_many.h"
#include "transcript_ops.h"
#include "verify_front.h"
#include "vkset_dev.h"
#include "vm_arena.h"
#include "g2_host.h"
#include "circuit.h"
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>

namespace plk {

constexpr uint32_t VM_PROOF_PTS = 11;                              // points a proof brings: wires 4, grand product, quotient 4, W_z, W_zw
constexpr uint32_t VM_NORM_K = 8;
constexpr uint32_t VM_PAIR_THREADS = 64;                           // one wave per workgroup: a small batch still spreads over the CUs
constexpr uint64_t VM_CHUNK = 1u << 16;                            // proofs per pass through the staging arena (5.5 KB each)

// term t of proof p: 0..10 the key's commitments and 22 the generator (fixed[0..11]); 11..21 the proof's points; 23, 24 = W_z, W_zw again
__device__ __forceinline__ const G1Affine *vm_term_point(const G1Affine *fixed, const G1Affine *pts, uint32_t p, uint32_t t) {
    if (t < 11) return fixed + t;
    if (t < 22) return pts + (size_t)p * VM_PROOF_PTS + (t - 11);
    if (t == 22) return fixed + 11;
    return pts + (size_t)p * VM_PROOF_PTS + (t - 23 + 9);
}

__global__ void __launch_bounds__(G1NTT_THREADS, 1) vm_mul_kernel(XyzzW *prod, const G1Affine *fixed, const G1Affine *pts, const Fr *sc, uint32_t m) {
    extern __shared__ uint32_t g1tab[];
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m * (uint32_t)VERIFY_TERMS) return;
    const uint32_t p = j / VERIFY_TERMS, t = j % VERIFY_TERMS;
    const G1Affine a = load_affine(vm_term_point(fixed, pts, p, t));
    XyzzW b = xyzzw_identity();
    if (!is_inf(a)) {
        b.x = csub_p(w_from_s(unpack<FqW>(a.x))); b.y = csub_p(w_from_s(unpack<FqW>(a.y)));
        b.zz = w_one<FqW>(); b.zzz = w_one<FqW>();
    }
    const Fr k = to_canonical(load_fp(sc + j));                   // the header's scalars are canonical, the ABI's are Montgomery
    store_xyzzw(prod + j, g1_mul_scalar_iso(b, k, g1tab));
}

__global__ void __launch_bounds__(256) vm_sum_kernel(G1Xyzz *sums, const XyzzW *prod, uint32_t m) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * m) return;
    const uint32_t p = j >> 1, lo = (j & 1) ? VERIFY_TERMS_PG : 0, hi = (j & 1) ? VERIFY_TERMS : VERIFY_TERMS_PG;
    const XyzzW *src = prod + (size_t)p * VERIFY_TERMS;
    XyzzW acc = load_xyzzw(src + lo);
    for (uint32_t k = lo + 1; k < hi; k++) { const XyzzW b = load_xyzzw(src + k); g1_add_call(&acc, &b); }
    store_xyzz(sums + j, xyzzw_export(acc));
}

__global__ void __launch_bounds__(256) vm_affine_kernel(G1Affine *out, const G1Xyzz *in, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lo = t * VM_NORM_K, hi = lo + VM_NORM_K < n ? lo + VM_NORM_K : n;
    if (lo >= n) return;
    Fq prefix[VM_NORM_K];
    Fq acc = Fq::one();
#pragma unroll
    for (uint32_t j = 0; j < VM_NORM_K; j++) {
        if (lo + j < hi) { const Fq z = load_fp(&in[lo + j].zzz); if (!z.is_zero()) acc = mul(acc, z); }
        prefix[j] = acc;
    }
    Fq inv_acc = inv(acc);
#pragma unroll
    for (uint32_t jj = 0; jj < VM_NORM_K; jj++) {
        const uint32_t j = VM_NORM_K - 1 - jj;
        if (lo + j >= hi) continue;
        const G1Xyzz q = load_xyzz(in + lo + j);
        G1Affine a; a.x = Fq::zero(); a.y = Fq::zero();
        if (!is_inf(q)) {
            const Fq zi = j ? mul(inv_acc, prefix[j - 1]) : inv_acc;  // 1 / ZZZ_j
            inv_acc = mul(inv_acc, q.zzz);
            const Fq iz = mul(q.zz, zi), izz = mul(iz, iz);       // 1 / Z, 1 / ZZ
            a.x = mul(q.x, izz);
            a.y = mul(q.y, zi);
        }
        store_fp(&out[lo + j].x, a.x);
        store_fp(&out[lo + j].y, a.y);
    }
}

// verdict[i] = 1 / 0: e(a_i, Q0) e(b_i, Q1) is / is not 1;  2: a_i or b_i is not on the curve.  a_i = a[i * stride], b_i = b[i * stride]
__global__ void __launch_bounds__(VM_PAIR_THREADS) vm_pairing_kernel(uint8_t *verdict, const G1Affine *a, const G1Affine *b, uint32_t stride, uint32_t n,
                                                                     const PairingHead *head, const Fq *lines) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Affine A = load_affine(a + (size_t)i * stride), B = load_affine(b + (size_t)i * stride);
    uint8_t v = 2;
    if (fq_on_curve(A.x, A.y) && fq_on_curve(B.x, B.y)) v = pairing_is_one_from_lines(A.x, A.y, B.x, B.y, head, lines) ? 1 : 0;
    verdict[i] = v;
}

// [PairingHead | lines | fixed points] in one device allocation
static size_t table_bytes(uint32_t lines) { return sizeof(PairingHead) + (size_t)lines * 8 * sizeof(Fq); }
static_assert(sizeof(PairingHead) % 16 == 0, "the line table behind the head must stay 16-byte aligned");

static int32_t pairing_launch(uint8_t *verdict, const G1Affine *a, const G1Affine *b, uint32_t stride, uint32_t n, const void *table, hipStream_t st) {
    const PairingHead *head = reinterpret_cast<const PairingHead *>(table);
    const Fq *lines = reinterpret_cast<const Fq *>(reinterpret_cast<const char *>(table) + sizeof(PairingHead));
    hipLaunchKernelGGL(vm_pairing_kernel, dim3((n + VM_PAIR_THREADS - 1) / VM_PAIR_THREADS), dim3(VM_PAIR_THREADS), 0, st, verdict, a, b, stride, n, head, lines);
    PLK_HIP(hipGetLastError());
    return PLK_OK;
}

// ---- a key set (plk_vkset): the same kernels with the key taken per lane through vkset_lookup (vkset_dev.h).  NO COUNTERPART IN THE REFERENCE.
// vm_mul_kernel's body with terms 0..10 and 22 of proof p taken from key key_of[p].  A key index out of range (plk_verify_mixed_dev only: the
// front kernel settled that proof as malformed and zeroed its scalars) reads no key and multiplies the identity.
__global__ void __launch_bounds__(G1NTT_THREADS, 1) vm_mul_mixed_kernel(XyzzW *prod, VksetView set, const uint32_t *key_of, const G1Affine *pts, const Fr *sc, uint32_t m) {
    extern __shared__ uint32_t g1tab[];
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m * (uint32_t)VERIFY_TERMS) return;
    const uint32_t p = j / VERIFY_TERMS, t = j % VERIFY_TERMS;
    VksetKey key;
    key.fixed = nullptr;                                           // one load site below, as in vm_mul_kernel (the compiler)
    const bool have = (t < 11 || t == 22) ? vkset_lookup(set, key_of[p], &key) : true;
    G1Affine a; a.x = Fq::zero(); a.y = Fq::zero();
    if (have) a = load_affine(vm_term_point(key.fixed, pts, p, t));
    XyzzW b = xyzzw_identity();
    if (!is_inf(a)) {
        b.x = csub_p(w_from_s(unpack<FqW>(a.x))); b.y = csub_p(w_from_s(unpack<FqW>(a.y)));
        b.zz = w_one<FqW>(); b.zzz = w_one<FqW>();
    }
    const Fr k = to_canonical(load_fp(sc + j));
    store_xyzzw(prod + j, g1_mul_scalar_iso(b, k, g1tab));
}

// vm_pairing_kernel with head and lines of lane i's key: the lanes of a wave may walk different tables, and q_inf (so the on[] tests of
// pairing_is_one_from_lines) may differ from lane to lane.  Launched only when the set holds more than one table.
__global__ void __launch_bounds__(VM_PAIR_THREADS) vm_pairing_mixed_kernel(uint8_t *verdict, const G1Affine *a, const G1Affine *b, uint32_t stride, uint32_t n, VksetView set,
                                                                           const uint32_t *key_of) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Affine A = load_affine(a + (size_t)i * stride), B = load_affine(b + (size_t)i * stride);
    uint8_t v = 2;
    VksetKey key;
    if (vkset_lookup(set, key_of[i], &key) && fq_on_curve(A.x, A.y) && fq_on_curve(B.x, B.y))
        v = pairing_is_one_from_lines(A.x, A.y, B.x, B.y, key.head, key.lines) ? 1 : 0;
    verdict[i] = v;
}

}  // namespace plk

using namespace plk;

struct plk_vk {
    int device = 0;
    uint32_t flags = 0;
    ParsedVk *parsed = nullptr;
    void *dev = nullptr;                                           // [PairingHead | lines | 12 fixed points | FrontVk]
    size_t fixed_off = 0, front_off = 0;
};

extern "C" void plk_vk_free(plk_vk *vk) {
    if (!vk) return;
    if (vk->dev) { (void)hipSetDevice(vk->device); (void)hipFree(vk->dev); }
    parsed_vk_free(vk->parsed);
    delete vk;
}

extern "C" int32_t plk_vk_load(plk_ctx *ctx, const uint8_t *vk_bytes, uint64_t len, uint32_t flags, plk_vk **out) {
    if (!ctx || !vk_bytes || !out) { set_error("plk_vk_load: null argument"); return PLK_ERR_ARG; }
    if (flags & ~(uint32_t)PLK_VERIFY_STRICT_INPUTS) { set_error("plk_verify_ex: unknown flag"); return PLK_ERR_ARG; }
    ParsedVk *parsed = parsed_vk_new(vk_bytes, len);
    if (!parsed) { set_error("plk_verify: malformed verification key"); return PLK_ERR_ARG; }
    plk_vk *vk = new plk_vk;
    vk->device = ctx->device; vk->flags = flags; vk->parsed = parsed;
    plk_g1_affine fixed[VERIFY_FIXED]; host::G2Affine g2[2];
    parsed_vk_points(parsed, fixed, g2);
    PairingHead head; std::vector<Fq> lines;
    make_pairing_table(g2, &head, &lines);
    vk->fixed_off = table_bytes(head.lines);
    vk->front_off = vk->fixed_off + sizeof fixed;
    static_assert(sizeof fixed % 16 == 0 && sizeof(FrontVk) % 16 == 0, "FrontVk behind the fixed points must stay 16-byte aligned");
    FrontVk front;                                                 // what vm_front_kernel needs from the key: sizes, flags, non-residues, omega
    memset(&front, 0, sizeof front);
    {
        plk_fr nr[3], om;
        parsed_vk_front(parsed, &front.n, &front.num_inputs, nr, &om);
        front.flags = flags;
        memcpy(front.non_residues, nr, sizeof nr); memcpy(&front.omega, &om, sizeof om);
    }
    std::vector<uint8_t> img(vk->front_off + sizeof front);
    memcpy(img.data(), &head, sizeof head);
    memcpy(img.data() + sizeof head, lines.data(), lines.size() * sizeof(Fq));
    memcpy(img.data() + vk->fixed_off, fixed, sizeof fixed);
    memcpy(img.data() + vk->front_off, &front, sizeof front);
    int32_t rc = [&]() -> int32_t {
        PLK_HIP(hipSetDevice(ctx->device));
        PLK_HIP(hipMalloc(&vk->dev, img.size()));
        PLK_HIP(hipMemcpy(vk->dev, img.data(), img.size(), hipMemcpyHostToDevice));
        return PLK_OK;
    }();
    if (rc != PLK_OK) { plk_vk_free(vk); return rc; }
    *out = vk;
    return PLK_OK;
}

extern "C" int32_t plk_pairing_check_many_dev(plk_ctx *ctx, const void *a_dev, const void *b_dev, uint64_t n, const uint8_t g2[256], void *verdict_dev, void *stream) {
    if (!ctx || !g2 || (n && (!a_dev || !b_dev || !verdict_dev))) { set_error("plk_pairing_check_many_dev: null argument"); return PLK_ERR_ARG; }
    if (((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)verdict_dev) & 15) { set_error("plk_pairing_check_many_dev: device pointers must be 16-byte aligned"); return PLK_ERR_ARG; }
    if (n > (1ull << 28)) { set_error("plk_pairing_check_many_dev: more than 2^28 checks"); return PLK_ERR_SIZE; }
    host::G2Affine q[2];
    if (!host::g2_from_bytes(g2, &q[0]) || !host::g2_from_bytes(g2 + 128, &q[1])) { set_error("plk_pairing_check: G2 point not on the twist"); return PLK_ERR_ARG; }
    if (n == 0) return PLK_OK;
    PLK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (!ctx->pair_tab_valid || memcmp(ctx->pair_g2, g2, 256) != 0) {
        // a new G2 pair: its table replaces the last one's, which kernels already on `st` may still read
        PairingHead head; std::vector<Fq> lines;
        make_pairing_table(q, &head, &lines);
        std::vector<uint8_t> img(table_bytes(head.lines));
        memcpy(img.data(), &head, sizeof head);
        memcpy(img.data() + sizeof head, lines.data(), lines.size() * sizeof(Fq));
        ctx->pair_tab_valid = false;
        PLK_HIP(hipStreamSynchronize(st));
        PLK_TRY(ctx->pair_tab.reserve(img.size()));
        PLK_HIP(hipMemcpy(ctx->pair_tab.p, img.data(), img.size(), hipMemcpyHostToDevice));
        memcpy(ctx->pair_g2, g2, 256);
        ctx->pair_tab_valid = true;
    }
    return pairing_launch(reinterpret_cast<uint8_t *>(verdict_dev), reinterpret_cast<const G1Affine *>(a_dev), reinterpret_cast<const G1Affine *>(b_dev), 1, (uint32_t)n,
                          ctx->pair_tab.p, st);
}

// ---- a key set for a mixed batch: proofs of several verification keys in one pass (plk_vkset_create, plk_verify_mixed, _packed, _dev).
// NO COUNTERPART IN THE REFERENCE.  Verdict i is what plk_verify_ex says about proof i under key key_of[i]: the single-key calls with the key
// taken per proof.  The front kernel, the scalar multiplications and (when the set holds more than one G2 pair) the pairing kernel go through
// vkset_lookup; the sums, XYZZ -> affine and the settling are the kernels above, unchanged.
static_assert(VKSET_MAX_KEYS == PLK_VKSET_MAX_KEYS, "vkset_plan.h restates the header's bound");

struct plk_vkset {
    int device = 0;
    std::vector<ParsedVk *> parsed;                                // per key, copies of the set's own
    std::vector<uint32_t> flags;
    VksetLayout layout;
    VksetView view;                                                // device pointers into `dev`
    void *dev = nullptr;                                           // the image of vkset_plan.h
};

extern "C" void plk_vkset_free(plk_vkset *set) {
    if (!set) return;
    if (set->dev) { (void)hipSetDevice(set->device); (void)hipFree(set->dev); }
    for (ParsedVk *p : set->parsed) parsed_vk_free(p);
    delete set;
}

extern "C" uint32_t plk_vkset_keys(const plk_vkset *set) { return set ? set->layout.n_keys : 0; }
extern "C" uint32_t plk_vkset_tables(const plk_vkset *set) { return set ? set->layout.n_tables : 0; }

static int32_t vkset_create_body(plk_ctx *ctx, const plk_vk *const *keys, uint32_t n_keys, plk_vkset **out) {
    if (!ctx || !keys || !out) { set_error("plk_vkset_create: null argument"); return PLK_ERR_ARG; }
    if (n_keys == 0 || n_keys > VKSET_MAX_KEYS) { set_error("plk_vkset_create: a set holds 1 to " + std::to_string(VKSET_MAX_KEYS) + " keys"); return PLK_ERR_ARG; }
    for (uint32_t k = 0; k < n_keys; k++) {
        if (!keys[k]) { set_error("plk_vkset_create: null argument"); return PLK_ERR_ARG; }
        if (keys[k]->device != ctx->device) { set_error("plk_vkset_create: a verification key was loaded on another device"); return PLK_ERR_ARG; }
    }
    std::vector<uint8_t> g2((size_t)n_keys * VKSET_G2_BYTES);
    for (uint32_t k = 0; k < n_keys; k++) {                          // the key's G2 pair in the file encoding, from the parsed key
        plk_g1_affine fixed[VERIFY_FIXED]; host::G2Affine q[2];
        parsed_vk_points(keys[k]->parsed, fixed, q);
        host::g2_to_bytes(q[0], &g2[(size_t)k * VKSET_G2_BYTES]); host::g2_to_bytes(q[1], &g2[(size_t)k * VKSET_G2_BYTES + 128]);
    }
    std::vector<uint32_t> table_of, first_key;
    const uint32_t n_tables = vkset_dedup(g2.data(), n_keys, &table_of, &first_key);
    // the tables are rebuilt as plk_vk_load built them; the line count does not depend on the pair
    std::vector<PairingHead> heads(n_tables);
    std::vector<std::vector<Fq>> lines(n_tables);
    for (uint32_t t = 0; t < n_tables; t++) {
        plk_g1_affine fixed[VERIFY_FIXED]; host::G2Affine q[2];
        parsed_vk_points(keys[first_key[t]]->parsed, fixed, q);
        make_pairing_table(q, &heads[t], &lines[t]);
        if (heads[t].lines != heads[0].lines || lines[t].size() != (size_t)heads[0].lines * 8) { set_error("plk_vkset_create: line tables of different lengths"); return PLK_ERR_HIP; }
    }
    std::unique_ptr<plk_vkset, void (*)(plk_vkset *)> owner(new plk_vkset, plk_vkset_free);   // freed with its cloned keys on every way out but the last
    plk_vkset *set = owner.get();
    set->device = ctx->device;
    set->layout = vkset_layout(n_keys, n_tables, table_bytes(heads[0].lines));
    const VksetLayout &L = set->layout;
    std::vector<uint8_t> img(L.bytes, 0);
    for (uint32_t k = 0; k < n_keys; k++) {
        const plk_vk *vk = keys[k];
        set->parsed.push_back(parsed_vk_clone(vk->parsed));
        set->flags.push_back(vk->flags);
        plk_g1_affine fixed[VERIFY_FIXED]; host::G2Affine q[2];
        parsed_vk_points(vk->parsed, fixed, q);
        FrontVk front;
        memset(&front, 0, sizeof front);
        plk_fr nr[3], om;
        parsed_vk_front(vk->parsed, &front.n, &front.num_inputs, nr, &om);
        front.flags = vk->flags;
        memcpy(front.non_residues, nr, sizeof nr); memcpy(&front.omega, &om, sizeof om);
        memcpy(img.data() + L.front_off + (size_t)k * VKSET_FRONT_BYTES, &front, sizeof front);
        memcpy(img.data() + L.fixed_off + (size_t)k * VKSET_FIXED_BYTES, fixed, sizeof fixed);
        memcpy(img.data() + L.index_off + (size_t)k * sizeof(uint32_t), &table_of[k], sizeof(uint32_t));
    }
    for (uint32_t t = 0; t < n_tables; t++) {
        uint8_t *at = img.data() + L.tables_off + (size_t)t * L.table_stride;
        memcpy(at, &heads[t], sizeof(PairingHead));
        memcpy(at + sizeof(PairingHead), lines[t].data(), lines[t].size() * sizeof(Fq));
    }
    const int32_t rc = [&]() -> int32_t {
        PLK_HIP(hipSetDevice(ctx->device));
        PLK_HIP(hipMalloc(&set->dev, img.size()));
        PLK_HIP(hipMemcpy(set->dev, img.data(), img.size(), hipMemcpyHostToDevice));
        return PLK_OK;
    }();
    if (rc != PLK_OK) return rc;
    set->view = vkset_view(set->dev, L);
    *out = owner.release();
    return PLK_OK;
}

extern "C" int32_t plk_vkset_create(plk_ctx *ctx, const plk_vk *const *keys, uint32_t n_keys, plk_vkset **out) {
    return guarded("plk_vkset_create", PLK_ERR_ARG, [&] { return vkset_create_body(ctx, keys, n_keys, out); });
}

// ---- the working memory of a pass: the layout of vm_arena.h over a block of the device
static_assert(VM_ARENA_PTS == VM_PROOF_PTS && VM_ARENA_TERMS == VERIFY_TERMS, "vm_arena.h restates the counts");
static_assert(sizeof(G1Affine) == VM_AFFINE_BYTES && sizeof(Fr) == VM_FR_BYTES && sizeof(XyzzW) == VM_XYZZW_BYTES && sizeof(G1Xyzz) == VM_XYZZ_BYTES, "vm_arena.h sizes the parts");

struct VmArena {
    G1Affine *pts; Fr *sc; XyzzW *prod; G1Xyzz *sum; G1Affine *aff; uint8_t *v, *state; uint32_t *keys; uint64_t *off; uint8_t *blob;
    VmArena(const DevBuf &buf, const VmLayout &L) {
        char *d = buf.as<char>();
        pts = reinterpret_cast<G1Affine *>(d + L.pts); sc = reinterpret_cast<Fr *>(d + L.sc); prod = reinterpret_cast<XyzzW *>(d + L.prod);
        sum = reinterpret_cast<G1Xyzz *>(d + L.sum); aff = reinterpret_cast<G1Affine *>(d + L.aff);
        v = reinterpret_cast<uint8_t *>(d + L.v); state = reinterpret_cast<uint8_t *>(d + L.state);
        keys = reinterpret_cast<uint32_t *>(d + L.keys); off = reinterpret_cast<uint64_t *>(d + L.off); blob = reinterpret_cast<uint8_t *>(d + L.blob);
    }
};

// where a pass whose front end runs on the device finds its proofs: proof i is blob[off[i] - bias, off[i + 1] - bias), blob_len bytes in all
struct VmRaw { const uint8_t *blob; uint64_t blob_len; const uint64_t *off; uint64_t bias; };

// ---- whose proofs these are: one key, or a key set with a key index per proof.  What differs between plk_verify_many* and plk_verify_mixed*
// is answered here; the pass and the three drivers below serve both.
struct VmKeys {
    const plk_vk *vk = nullptr;
    const plk_vkset *set = nullptr;
    const uint32_t *key_of = nullptr;                              // a set: the key index per proof, in host memory (blocking calls) or on the device (_dev)
    explicit VmKeys(const plk_vk *k) : vk(k) {}
    VmKeys(const plk_vkset *s, const uint32_t *ko) : set(s), key_of(ko) {}
    bool missing(uint64_t count) const { return set ? count && !key_of : !vk; }
    int device() const { return set ? set->device : vk->device; }
    const ParsedVk *parsed(uint64_t i) const { return set ? set->parsed[key_of[i]] : vk->parsed; }   // host front end, key_of on the host
    uint32_t flags(uint64_t i) const { return set ? set->flags[key_of[i]] : vk->flags; }
    const G1Affine *fixed() const { return reinterpret_cast<const G1Affine *>(reinterpret_cast<const char *>(vk->dev) + vk->fixed_off); }
    const FrontVk *front_vk() const { return reinterpret_cast<const FrontVk *>(reinterpret_cast<const char *>(vk->dev) + vk->front_off); }

    // the refusals every call shares
    int32_t guard(const char *who, const plk_ctx *ctx) const {
        if (device() != ctx->device) {
            set_error(std::string(who) + (set ? ": the key set was made on another device" : ": the verification key was loaded on another device"));
            return PLK_ERR_ARG;
        }
        if (ctx->msm_enq != ctx->msm_fin) { set_error(std::string(who) + ": a commitment enqueued with plk_msm_g1_enqueue_dev is still in flight (call plk_msm_g1_finish first)"); return PLK_ERR_ARG; }
        return PLK_OK;
    }
    // key_of on the host: every index names a key of the set
    int32_t indices_ok(const char *who, uint64_t count) const {
        uint64_t bad = 0;
        if (!set || vkset_indices_ok(key_of, count, set->layout.n_keys, &bad)) return PLK_OK;
        set_error(std::string(who) + ": key_of[" + std::to_string(bad) + "] = " + std::to_string(key_of[bad]) + " but the set holds " + std::to_string(set->layout.n_keys) + " keys");
        return PLK_ERR_ARG;
    }

    // the three keyed steps of a pass over m proofs; d_key: the pass's key indices on the device (a set only)
    int32_t front(const VmArena &A, const VmRaw &R, const uint32_t *d_key, uint32_t m, hipStream_t st) const {
        if (set) return front_mixed_launch(A.pts, A.sc, A.state, R.blob, R.blob_len, R.off, R.bias, m, set->view, d_key, st);
        return front_launch(A.pts, A.sc, A.state, R.blob, R.blob_len, R.off, R.bias, m, front_vk(), fixed(), false, st);
    }
    int32_t mul(const VmArena &A, const uint32_t *d_key, uint32_t m, hipStream_t st) const {
        static std::atomic<bool> attr_set{false};
        if (!attr_set) {
            PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vm_mul_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO));
            PLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vm_mul_mixed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G1NTT_LDS_ISO));
            attr_set = true;
        }
        const dim3 grid((m * (uint32_t)VERIFY_TERMS + G1NTT_THREADS - 1) / G1NTT_THREADS), block(G1NTT_THREADS);
        if (set) hipLaunchKernelGGL(vm_mul_mixed_kernel, grid, block, G1NTT_LDS_ISO, st, A.prod, set->view, d_key, (const G1Affine *)A.pts, (const Fr *)A.sc, m);
        else hipLaunchKernelGGL(vm_mul_kernel, grid, block, G1NTT_LDS_ISO, st, A.prod, fixed(), (const G1Affine *)A.pts, (const Fr *)A.sc, m);
        PLK_HIP(hipGetLastError());
        return PLK_OK;
    }
    // one G2 pair in the set (the common case: keys of one universal key): the single-key kernel, whose line loads are wave-uniform
    int32_t pairing(const VmArena &A, const uint32_t *d_key, uint32_t m, hipStream_t st) const {
        if (!set || set->layout.n_tables == 1) return pairing_launch(A.v, A.aff, A.aff + 1, 2, m, set ? (const void *)set->view.tables : vk->dev, st);
        hipLaunchKernelGGL(vm_pairing_mixed_kernel, dim3((m + VM_PAIR_THREADS - 1) / VM_PAIR_THREADS), dim3(VM_PAIR_THREADS), 0, st, A.v, (const G1Affine *)A.aff,
                           (const G1Affine *)(A.aff + 1), 2u, m, set->view, d_key);
        PLK_HIP(hipGetLastError());
        return PLK_OK;
    }
};

// ---- one pass over the m proofs of arena A, enqueued on st: [the front kernel over R,] the scalar multiplications, the sums, XYZZ -> affine,
// the pairing [, and the verdicts settled from the state bytes into d_out].  With R every proof of the pass goes through the kernels, a proof
// the front end settled as 25 zero terms (its sums are the identity).  Without R the host front end has filled A.pts and A.sc with the proofs
// that passed it, and the pairing verdicts stay in A.v.  Marks k .. k + 2, or k .. k + 3 with R, behind front | mul | sums, affine | the rest.
using VmTimer = StageTimer<7>;

static int32_t vm_pass(const VmKeys &K, const VmArena &A, const uint32_t *d_key, uint32_t m, const VmRaw *R, uint8_t *d_out, hipStream_t st, VmTimer &ev, int k) {
    if (R) { PLK_TRY(K.front(A, *R, d_key, m, st)); PLK_TRY(ev.mark(k++, st)); }
    PLK_TRY(K.mul(A, d_key, m, st));
    PLK_TRY(ev.mark(k, st));
    hipLaunchKernelGGL(vm_sum_kernel, dim3((2 * m + 255) / 256), dim3(256), 0, st, A.sum, (const XyzzW *)A.prod, m);
    hipLaunchKernelGGL(vm_affine_kernel, dim3(((2 * m + VM_NORM_K - 1) / VM_NORM_K + 255) / 256), dim3(256), 0, st, A.aff, (const G1Xyzz *)A.sum, 2 * m);
    PLK_HIP(hipGetLastError());
    PLK_TRY(ev.mark(k + 1, st));
    PLK_TRY(K.pairing(A, d_key, m, st));
    if (R) PLK_TRY(settle_launch(d_out, A.v, A.state, m, st));
    return ev.mark(k + 2, st);
}

// plk_verify_many_last_ms: [0] host flattening, or the front kernel; [1] upload; [2] scalar multiplications; [3] sums and affine; [4] pairing
// (with settle); [5] download.  A blocking pass marks 0 | upload | 1 | vm_pass from 2 | download | last: its times are added to ms here.
static int32_t vm_add_times(VmTimer &ev, bool front_kernel, float ms[6]) {
    if (!ev.on) return PLK_OK;
    const int f = front_kernel ? 1 : 0;
    float t = 0;
    PLK_TRY(ev.elapsed(0, 1, &t)); ms[1] += t;
    if (f) { PLK_TRY(ev.elapsed(1, 2, &t)); ms[0] += t; }
    for (int s = 2; s < 6; s++) { PLK_TRY(ev.elapsed(s - 1 + f, s + f, &t)); ms[s] += t; }
    return PLK_OK;
}

static void vm_times_done(plk_ctx *ctx, const VmTimer &ev, const float ms[6]) {
    if (ev.on) { memcpy(ctx->vm_ms, ms, 6 * sizeof(float)); ctx->vm_ms_valid = true; }
}

static void vm_first_bad(const uint8_t *verdict, uint64_t count, uint64_t *first_bad) {
    for (uint64_t i = 0; i < count; i++) if (verdict[i] != 1) { *first_bad = i; break; }
}

// ---- driver 1, the host front end (plk_verify_many, _with, plk_verify_mixed).  Per chunk, on up to 16 threads: every proof through
// plk_verify_terms's code under its own key; the survivors are packed in index order (with their keys) and go through a pass.
// ops: the caller's transcript (plk_verify_many_with), null for Keccak.  Without PLK_TRANSCRIPT_CONCURRENT the front end then stays on the
// calling thread, one proof after the other, and the lowest proof that met a failure of the transcript ends the call.
static int32_t vm_run_host(plk_ctx *ctx, const VmKeys &K, const uint8_t *const *proofs, const uint64_t *lens, uint64_t count, uint8_t *verdict, const plk_transcript_ops *ops) {
    using clk = std::chrono::steady_clock;
    VmTimer ev;
    ctx->vm_ms_valid = false;
    float ms[6] = {0, 0, 0, 0, 0, 0};
    hipStream_t st = ctx->stream;
    PLK_TRY(ev.start(ctx));
    std::vector<plk_g1_affine> h_pts;
    std::vector<plk_fr> h_sc;
    std::vector<uint64_t> live;
    std::vector<uint32_t> live_key;
    std::vector<uint8_t> h_v;
    for (uint64_t base = 0; base < count; base += VM_CHUNK) {
        const uint64_t cnt = count - base < VM_CHUNK ? count - base : VM_CHUNK;
        const auto t0 = clk::now();
        std::vector<plk_g1_affine> all_pts((size_t)cnt * VM_PROOF_PTS);
        std::vector<plk_fr> all_sc((size_t)cnt * VERIFY_TERMS);
        const unsigned front_threads = ops && !(ops->flags & PLK_TRANSCRIPT_CONCURRENT) ? 1 : 16;
        std::mutex tr_mu;
        uint64_t tr_bad = UINT64_MAX; int32_t tr_rc = PLK_OK; std::string tr_words;
        parallel_for((size_t)cnt, 1, [&](size_t lo, size_t hi) {
            plk_g1_affine pts[VERIFY_TERMS]; plk_fr sc[VERIFY_TERMS];
            std::string msg;
            for (size_t i = lo; i < hi; i++) {
                int32_t early = 0;
                if (front_threads == 1 && tr_rc != PLK_OK) break;      // (one thread: nothing else writes tr_rc) no further begin after a failure
                const int32_t rc = verify_terms_parsed(K.parsed(base + i), proofs[base + i], lens[base + i], K.flags(base + i), pts, sc, &early, ops, &msg);
                if (rc != PLK_OK && !msg.empty()) {
                    std::lock_guard<std::mutex> g(tr_mu);
                    if (base + i < tr_bad) { tr_bad = base + i; tr_rc = rc; tr_words = msg; }
                    msg.clear(); verdict[base + i] = 0; continue;
                }
                if (rc != PLK_OK) { verdict[base + i] = PLK_VERDICT_MALFORMED; continue; }
                if (!early) { verdict[base + i] = 0; continue; }
                verdict[base + i] = 0xff;                             // goes to the device
                memcpy(&all_pts[i * VM_PROOF_PTS], &pts[11], VM_PROOF_PTS * sizeof(plk_g1_affine));
                memcpy(&all_sc[i * VERIFY_TERMS], sc, sizeof sc);
            }
        }, front_threads);
        if (tr_rc != PLK_OK) { set_error("plk_verify_many_with: proof " + std::to_string(tr_bad) + ": " + tr_words); return tr_rc; }
        if (K.set) vkset_compact(verdict + base, K.key_of + base, cnt, &live, &live_key);
        else { live.clear(); for (uint64_t i = 0; i < cnt; i++) if (verdict[base + i] == 0xff) live.push_back(i); }
        const uint32_t m = (uint32_t)live.size();
        h_pts.resize((size_t)m * VM_PROOF_PTS); h_sc.resize((size_t)m * VERIFY_TERMS); h_v.resize(m);
        for (uint32_t k = 0; k < m; k++) {
            memcpy(&h_pts[(size_t)k * VM_PROOF_PTS], &all_pts[live[k] * VM_PROOF_PTS], VM_PROOF_PTS * sizeof(plk_g1_affine));
            memcpy(&h_sc[(size_t)k * VERIFY_TERMS], &all_sc[live[k] * VERIFY_TERMS], VERIFY_TERMS * sizeof(plk_fr));
        }
        ms[0] += std::chrono::duration<float, std::milli>(clk::now() - t0).count();
        if (!m) continue;
        const VmLayout L = vm_layout(m, K.set != nullptr, false, 0);
        PLK_TRY(ctx->stage.reserve(L.bytes));
        const VmArena A(ctx->stage, L);
        PLK_TRY(ev.mark(0, st));
        PLK_HIP(hipMemcpyAsync(A.pts, h_pts.data(), h_pts.size() * sizeof(plk_g1_affine), hipMemcpyHostToDevice, st));
        PLK_HIP(hipMemcpyAsync(A.sc, h_sc.data(), h_sc.size() * sizeof(plk_fr), hipMemcpyHostToDevice, st));
        if (K.set) PLK_HIP(hipMemcpyAsync(A.keys, live_key.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        PLK_TRY(ev.mark(1, st));
        PLK_TRY(vm_pass(K, A, K.set ? A.keys : nullptr, m, nullptr, nullptr, st, ev, 2));
        PLK_HIP(hipMemcpyAsync(h_v.data(), A.v, m, hipMemcpyDeviceToHost, st));
        PLK_TRY(ev.mark(5, st));
        PLK_HIP(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < m; k++) verdict[base + live[k]] = h_v[k];
        PLK_TRY(vm_add_times(ev, false, ms));
    }
    vm_times_done(ctx, ev, ms);
    return PLK_OK;
}

static int32_t vm_call_host(const char *who, plk_ctx *ctx, const VmKeys &K, const uint8_t *const *proofs, const uint64_t *lens, uint64_t count, const plk_transcript_ops *ops,
                            uint8_t *verdict, uint64_t *first_bad) {
    return guarded(who, PLK_ERR_ARG, [&]() -> int32_t {
        if (!ctx || K.missing(count) || !verdict || !first_bad || (count && (!proofs || !lens))) { set_error(std::string(who) + ": null argument"); return PLK_ERR_ARG; }
        for (uint64_t i = 0; i < count; i++) if (!proofs[i]) { set_error(std::string(who) + ": null argument"); return PLK_ERR_ARG; }
        PLK_TRY(K.guard(who, ctx));
        PLK_TRY(K.indices_ok(who, count));
        *first_bad = UINT64_MAX;
        if (count == 0) return PLK_OK;
        PLK_HIP(hipSetDevice(ctx->device));
        PLK_TRY(vm_run_host(ctx, K, proofs, lens, count, verdict, ops));
        vm_first_bad(verdict, count, first_bad);
        return PLK_OK;
    });
}

extern "C" int32_t plk_verify_many(plk_ctx *ctx, const plk_vk *vk, const uint8_t *const *proofs, const uint64_t *lens, uint64_t count, uint8_t *verdict, uint64_t *first_bad) {
    return vm_call_host("plk_verify_many", ctx, VmKeys(vk), proofs, lens, count, nullptr, verdict, first_bad);
}

// plk_verify_many with the host front end under the caller's transcript (verifier::verify::<_, _, T>, src/plonk.rs:198-204, per proof)
extern "C" int32_t plk_verify_many_with(plk_ctx *ctx, const plk_vk *vk, const uint8_t *const *proofs, const uint64_t *lens, uint64_t count,
                                        const plk_transcript_ops *ops, uint8_t *verdict, uint64_t *first_bad) {
    if (!ops) return plk_verify_many(ctx, vk, proofs, lens, count, verdict, first_bad);
    if (!transcript_ops_complete(ops)) { set_error("plk_verify_many_with: the transcript table has a null callback"); return PLK_ERR_ARG; }
    if (ops->flags & ~(uint32_t)PLK_TRANSCRIPT_CONCURRENT) { set_error("plk_verify_many_with: unknown flag in the transcript table"); return PLK_ERR_ARG; }
    const plk_transcript_ops table = *ops;
    return vm_call_host("plk_verify_many", ctx, VmKeys(vk), proofs, lens, count, &table, verdict, first_bad);
}

extern "C" int32_t plk_verify_mixed(plk_ctx *ctx, const plk_vkset *set, const uint8_t *const *proofs, const uint64_t *lens, const uint32_t *key_of, uint64_t count,
                                    uint8_t *verdict, uint64_t *first_bad) {
    return vm_call_host("plk_verify_mixed", ctx, VmKeys(set, key_of), proofs, lens, count, nullptr, verdict, first_bad);
}

// ---- driver 2, packed bytes on the host (plk_verify_many_packed, plk_verify_mixed_packed): per chunk the offsets, the key indices and the raw
// bytes go up, the pass runs its front end on the device, and the settled verdicts come down.
static int32_t vm_run_packed(plk_ctx *ctx, const VmKeys &K, const uint8_t *blob, const uint64_t *off, uint64_t count, uint8_t *verdict) {
    VmTimer ev;
    ctx->vm_ms_valid = false;
    float ms[6] = {0, 0, 0, 0, 0, 0};
    hipStream_t st = ctx->stream;
    PLK_TRY(ev.start(ctx));
    for (uint64_t base = 0; base < count; base += VM_CHUNK) {
        const uint32_t cnt = (uint32_t)(count - base < VM_CHUNK ? count - base : VM_CHUNK);
        const uint64_t lo = off[base], bytes = off[base + cnt] - lo;
        const VmLayout L = vm_layout(cnt, K.set != nullptr, true, bytes);
        PLK_TRY(ctx->stage.reserve(L.bytes));
        const VmArena A(ctx->stage, L);
        PLK_TRY(ev.mark(0, st));
        PLK_HIP(hipMemcpyAsync(A.off, off + base, ((size_t)cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        if (K.set) PLK_HIP(hipMemcpyAsync(A.keys, K.key_of + base, (size_t)cnt * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (bytes) PLK_HIP(hipMemcpyAsync(A.blob, blob + lo, bytes, hipMemcpyHostToDevice, st));
        PLK_TRY(ev.mark(1, st));
        const VmRaw R{A.blob, bytes, A.off, lo};
        PLK_TRY(vm_pass(K, A, K.set ? A.keys : nullptr, cnt, &R, A.v, st, ev, 2));
        PLK_HIP(hipMemcpyAsync(verdict + base, A.v, cnt, hipMemcpyDeviceToHost, st));
        PLK_TRY(ev.mark(6, st));
        PLK_HIP(hipStreamSynchronize(st));
        PLK_TRY(vm_add_times(ev, true, ms));
    }
    vm_times_done(ctx, ev, ms);
    return PLK_OK;
}

static int32_t vm_call_packed(const char *who, plk_ctx *ctx, const VmKeys &K, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, uint64_t count, uint8_t *verdict,
                              uint64_t *first_bad) {
    return guarded(who, PLK_ERR_ARG, [&]() -> int32_t {
        if (!ctx || K.missing(count) || !verdict || !first_bad || (count && !off) || (blob_len && !blob)) { set_error(std::string(who) + ": null argument"); return PLK_ERR_ARG; }
        PLK_TRY(K.guard(who, ctx));
        for (uint64_t i = 0; i < count; i++)
            if (off[i] > off[i + 1] || off[i + 1] > blob_len) { set_error(std::string(who) + ": offsets decrease or reach past the blob"); return PLK_ERR_ARG; }
        PLK_TRY(K.indices_ok(who, count));
        *first_bad = UINT64_MAX;
        if (count == 0) return PLK_OK;
        PLK_HIP(hipSetDevice(ctx->device));
        PLK_TRY(vm_run_packed(ctx, K, blob, off, count, verdict));
        vm_first_bad(verdict, count, first_bad);
        return PLK_OK;
    });
}

extern "C" int32_t plk_verify_many_packed(plk_ctx *ctx, const plk_vk *vk, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, uint64_t count, uint8_t *verdict,
                                          uint64_t *first_bad) {
    return vm_call_packed("plk_verify_many_packed", ctx, VmKeys(vk), blob, blob_len, off, count, verdict, first_bad);
}

extern "C" int32_t plk_verify_mixed_packed(plk_ctx *ctx, const plk_vkset *set, const uint8_t *blob, uint64_t blob_len, const uint64_t *off, const uint32_t *key_of,
                                           uint64_t count, uint8_t *verdict, uint64_t *first_bad) {
    return vm_call_packed("plk_verify_mixed_packed", ctx, VmKeys(set, key_of), blob, blob_len, off, count, verdict, first_bad);
}

// ---- driver 3, bytes on the device (plk_verify_many_dev, plk_verify_mixed_dev; K.key_of is a device pointer).  The call does not wait: its
// arena is vm_stage and its passes run on the context's stream (on_ctx_stream, ctx.h).  No times are recorded.
static int32_t vm_call_dev(const char *who, plk_ctx *ctx, const VmKeys &K, const void *blob_dev, uint64_t blob_len, const void *off_dev, uint64_t count, void *verdict_dev,
                           void *stream) {
    return guarded(who, PLK_ERR_ARG, [&]() -> int32_t {
        if (!ctx || K.missing(count) || (count && (!off_dev || !verdict_dev)) || (blob_len && !blob_dev)) { set_error(std::string(who) + ": null argument"); return PLK_ERR_ARG; }
        if (!K.set && ((uintptr_t)off_dev & 7)) { set_error(std::string(who) + ": the offset table must be 8-byte aligned"); return PLK_ERR_ARG; }
        if (K.set && (((uintptr_t)off_dev & 7) || ((uintptr_t)K.key_of & 3))) { set_error(std::string(who) + ": the offset table must be 8-byte aligned, the key indices 4-byte aligned"); return PLK_ERR_ARG; }
        PLK_TRY(K.guard(who, ctx));
        if (count == 0) return PLK_OK;
        PLK_HIP(hipSetDevice(ctx->device));
        ctx->vm_ms_valid = false;
        const VmLayout L = vm_layout(count < VM_CHUNK ? (size_t)count : (size_t)VM_CHUNK, false, false, 0);
        PLK_TRY(ctx->vm_stage.reserve(L.bytes));
        return on_ctx_stream(ctx, stream ? (hipStream_t)stream : ctx->stream, [&](hipStream_t st) -> int32_t {
            VmTimer none;                                             // never started
            for (uint64_t base = 0; base < count; base += VM_CHUNK) {
                const uint32_t cnt = (uint32_t)(count - base < VM_CHUNK ? count - base : VM_CHUNK);
                const VmArena A(ctx->vm_stage, vm_layout(cnt, false, false, 0));
                const VmRaw R{reinterpret_cast<const uint8_t *>(blob_dev), blob_len, reinterpret_cast<const uint64_t *>(off_dev) + base, 0};
                PLK_TRY(vm_pass(K, A, K.set ? K.key_of + base : nullptr, cnt, &R, reinterpret_cast<uint8_t *>(verdict_dev) + base, st, none, 2));
            }
            return PLK_OK;
        });
    });
}

extern "C" int32_t plk_verify_many_dev(plk_ctx *ctx, const plk_vk *vk, const void *blob_dev, uint64_t blob_len, const void *off_dev, uint64_t count, void *verdict_dev,
                                       void *stream) {
    return vm_call_dev("plk_verify_many_dev", ctx, VmKeys(vk), blob_dev, blob_len, off_dev, count, verdict_dev, stream);
}

extern "C" int32_t plk_verify_mixed_dev(plk_ctx *ctx, const plk_vkset *set, const void *blob_dev, uint64_t blob_len, const void *off_dev, const void *key_of_dev,
                                        uint64_t count, void *verdict_dev, void *stream) {
    return vm_call_dev("plk_verify_mixed_dev", ctx, VmKeys(set, reinterpret_cast<const uint32_t *>(key_of_dev)), blob_dev, blob_len, off_dev, count, verdict_dev, stream);
}

// the front kernel alone, all 25 terms per proof into the caller's arrays, on the caller's stream
extern "C" int32_t plk_verify_front_dev(plk_ctx *ctx, const plk_vk *vk, const void *blob_dev, uint64_t blob_len, const void *off_dev, uint64_t count, void *points_dev,
                                        void *scalars_dev, void *state_dev, void *stream) {
    const char *who = "plk_verify_front_dev";
    return guarded(who, PLK_ERR_ARG, [&]() -> int32_t {
        if (!ctx || !vk || (count && (!off_dev || !points_dev || !scalars_dev || !state_dev)) || (blob_len && !blob_dev)) { set_error("plk_verify_front_dev: null argument"); return PLK_ERR_ARG; }
        if (((uintptr_t)off_dev & 7) || (((uintptr_t)points_dev | (uintptr_t)scalars_dev) & 15)) { set_error("plk_verify_front_dev: points and scalars must be 16-byte aligned, offsets 8-byte aligned"); return PLK_ERR_ARG; }
        if (count > (1ull << 26)) { set_error("plk_verify_front_dev: more than 2^26 proofs"); return PLK_ERR_SIZE; }
        const VmKeys K(vk);
        PLK_TRY(K.guard(who, ctx));
        if (count == 0) return PLK_OK;
        PLK_HIP(hipSetDevice(ctx->device));
        return front_launch(reinterpret_cast<G1Affine *>(points_dev), reinterpret_cast<Fr *>(scalars_dev), reinterpret_cast<uint8_t *>(state_dev),
                            reinterpret_cast<const uint8_t *>(blob_dev), blob_len, reinterpret_cast<const uint64_t *>(off_dev), 0, (uint32_t)count, K.front_vk(), K.fixed(), true,
                            stream ? (hipStream_t)stream : ctx->stream);
    });
}

extern "C" int32_t plk_verify_many_last_ms(plk_ctx *ctx, float out_ms[6]) {
    if (!ctx || !out_ms) { set_error("plk_verify_many_last_ms: null argument"); return PLK_ERR_ARG; }
    if (!ctx->vm_ms_valid) { set_error("plk_verify_many_last_ms: no timed plk_verify_many on this context (plk_set_kernel_timing)"); return PLK_ERR_ARG; }
    for (int k = 0; k < 6; k++) out_ms[k] = ctx->vm_ms[k];
    return PLK_OK;
}
