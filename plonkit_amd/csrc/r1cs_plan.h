// The device layout of an R1CS for the witness check of r1cs_check.hip, built once per circuit from R1cs::terms / off (circuit.h).
// Host code only: no HIP include, so a stand-alone program can check the plan (tests/host/r1cs_plan_check.cpp).
//
// What the reference does with the same data: CircomCircuit::synthesize (src/circom_circuit.rs:74-133) hands every constraint
// A_i * B_i = C_i to the constraint system, and SetupForProver::validate_witness (src/plonk.rs:127-129) asks whether the witness
// satisfies them.  Wire 0 is Index::Input(0) = CS::one() whatever the witness file holds at index 0 (:78,107-113).
//
// Layout
//   terms      {u32 wire, u32 coeff_index}, 8 bytes, in the order of the host structure (A_0, B_0, C_0, A_1, ...), with the same
//              3m + 1 offsets.  A Montgomery coefficient is 32 bytes and a circom circuit has a handful of distinct ones.
//   table      the distinct coefficients, Montgomery form.  table[0] = 1 and table[1] = r - 1 always (the kernels add or subtract
//              for those two indices without a product: circom's output is mostly +-1); the others in order of first appearance.
//              Built by hashing the four limbs; when every coefficient is distinct the table is as long as the term list.
//   work lists LC indices (3 i + side).  `short_lcs`: fewer than R1CS_LONG_LC_TERMS terms (empty ones included), one lane each;
//              `long_lcs`: the others, one wave each.  Both ascending, every LC in exactly one.
#pragma once
#include "circuit.h"
#include <string>
#include <unordered_map>
#include <vector>

namespace plk {

// An LC of at least this many terms is summed by a whole wave (64 lanes striding over the terms, then a 6-step tree); below it one
// lane walks it.  At 16 terms a wave's lanes still do a quarter of a term each on average — the gain is in the waves of SHORT
// LCs that no longer wait for one 60-term neighbour — and the tree (48 cross-lane moves, 6 additions) costs about what 6 terms cost.
constexpr uint32_t R1CS_LONG_LC_TERMS = 16;

struct R1csPlanTerm { uint32_t wire, coeff; };
static_assert(sizeof(R1csPlanTerm) == 8, "the uploaded term record");

struct R1csPlan {
    uint64_t num_constraints = 0, num_variables = 0;
    big_vector<R1csPlanTerm> terms;
    std::vector<uint64_t> off;                  // 3 * num_constraints + 1
    std::vector<HFr> table;
    std::vector<uint32_t> short_lcs, long_lcs;
};

struct R1csCoeffHash {
    size_t operator()(const HFr &a) const {
        uint64_t h = a.l[0] * 0x9e3779b97f4a7c15ull;
        for (int i = 1; i < 4; i++) h = (h ^ (h >> 29) ^ a.l[i]) * 0xbf58476d1ce4e5b9ull;
        return (size_t)(h ^ (h >> 32));
    }
};

// false (and *err) for what the check cannot represent: a term on a wire >= num_variables, 2^32 or more terms or LCs
inline bool r1cs_plan_build(const R1cs &r, R1csPlan *out, std::string *err, uint32_t long_terms = R1CS_LONG_LC_TERMS) {
    const size_t n_lc = r.off.size() - 1, n_terms = r.terms.size();
    if (n_lc % 3 != 0 || r.off[n_lc] != n_terms) { *err = "malformed R1CS: the offsets do not cover the terms"; return false; }
    if (n_lc >= 0xffffffffull || n_terms >= 0xffffffffull) { *err = "R1CS too large for the witness check (2^32 terms or linear combinations)"; return false; }
    out->num_constraints = n_lc / 3;
    out->num_variables = r.num_variables;
    out->off = r.off;
    out->terms.resize(n_terms);
    out->table.clear();
    out->table.push_back(HFr::one());
    out->table.push_back(-HFr::one());
    std::unordered_map<HFr, uint32_t, R1csCoeffHash> seen;
    seen.emplace(out->table[0], 0u);
    seen.emplace(out->table[1], 1u);
    const HFr one = out->table[0], minus_one = out->table[1];
    for (size_t k = 0; k < n_terms; k++) {
        const LcTerm &t = r.terms[k];
        if (t.wire >= r.num_variables) {
            *err = "malformed R1CS: a term names wire " + std::to_string(t.wire) + " but the circuit has " + std::to_string(r.num_variables) + " variables";
            return false;
        }
        uint32_t idx;
        if (t.coeff == one) idx = 0;                              // (the two common ones never reach the hash table)
        else if (t.coeff == minus_one) idx = 1;
        else {
            auto it = seen.find(t.coeff);
            if (it == seen.end()) { idx = (uint32_t)out->table.size(); out->table.push_back(t.coeff); seen.emplace(t.coeff, idx); }
            else idx = it->second;
        }
        out->terms[k] = R1csPlanTerm{t.wire, idx};
    }
    out->short_lcs.clear(); out->long_lcs.clear();
    for (size_t j = 0; j < n_lc; j++) {
        if (r.off[j + 1] < r.off[j]) { *err = "malformed R1CS: the offsets decrease"; return false; }
        (r.off[j + 1] - r.off[j] < long_terms ? out->short_lcs : out->long_lcs).push_back((uint32_t)j);
    }
    return true;
}

// the value of LC j of the plan under `witness` (num_variables elements), wire 0 read as the constant 1 — the arithmetic of the kernels
inline HFr r1cs_plan_lc_value(const R1csPlan &p, size_t j, const HFr *witness) {
    HFr acc = HFr::zero();
    for (uint64_t k = p.off[j]; k < p.off[j + 1]; k++) {
        const R1csPlanTerm &t = p.terms[k];
        const HFr v = t.wire == 0 ? HFr::one() : witness[t.wire];
        if (t.coeff == 0) acc = acc + v;
        else if (t.coeff == 1) acc = acc - v;
        else acc = acc + p.table[t.coeff] * v;
    }
    return acc;
}

// the verdict of the plan on the host, through the work lists as the device takes them: the lowest constraint with a * b != c,
// UINT64_MAX when every constraint holds
inline uint64_t r1cs_plan_check_host(const R1csPlan &p, const HFr *witness) {
    std::vector<HFr> lc(3 * p.num_constraints, HFr::zero());
    for (uint32_t j : p.short_lcs) lc[j] = r1cs_plan_lc_value(p, j, witness);
    for (uint32_t j : p.long_lcs) lc[j] = r1cs_plan_lc_value(p, j, witness);
    for (uint64_t i = 0; i < p.num_constraints; i++)
        if (lc[3 * i] * lc[3 * i + 1] != lc[3 * i + 2]) return i;
    return ~0ull;
}

}  // namespace plk
