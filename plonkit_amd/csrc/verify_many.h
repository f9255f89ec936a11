// What plk_vk_load / plk_verify_many (verify_many.hip) take from the host verifier (verify.cpp): the parsed key and the flattened form of
// verify_keccak's two pairing arguments.  verify.cpp stays pure host code (the sanitizer build compiles it without HIP).
#pragma once
#include "../../include/plonkit_amd.h"
#include "pairing.h"
#include <string>

namespace plk {

constexpr int VERIFY_TERMS = 25, VERIFY_TERMS_PG = 23, VERIFY_FIXED = 12;   // pg: 11 of the key + 11 of the proof + the generator; px: 2

struct ParsedVk;                                                   // opaque: verify.cpp's parsed key
ParsedVk *parsed_vk_new(const uint8_t *vk, uint64_t len);           // null: plk_verify_ex would say "malformed verification key"
void parsed_vk_free(ParsedVk *v);
ParsedVk *parsed_vk_clone(const ParsedVk *v);                       // a copy of its own (plk_vkset_create: the set outlives the keys it was made from)
// the 12 points that are the same for every proof (terms 0..10 and 22 of plk_verify_terms) and the key's G2 pair
void parsed_vk_points(const ParsedVk *v, plk_g1_affine fixed[VERIFY_FIXED], host::G2Affine g2[2]);
// what the device front end (verify_front_dev.h FrontVk) takes from the key: n, the input count, the non-residues and omega of the domain n + 1
void parsed_vk_front(const ParsedVk *v, uint64_t *n, uint64_t *num_inputs, plk_fr non_residues[3], plk_fr *omega);
// plk_verify_terms on a parsed key; PLK_ERR_ARG "plk_verify: malformed proof" exactly when plk_verify_ex says so
int32_t verify_terms_parsed(const ParsedVk *v, const uint8_t *proof, uint64_t len, uint32_t flags, plk_g1_affine points[VERIFY_TERMS],
                            plk_fr scalars[VERIFY_TERMS], int32_t *early, const plk_transcript_ops *ops = nullptr, std::string *tr_msg = nullptr);
// ops: the caller's transcript (null: Keccak).  Its failure is the return code, with the words in *tr_msg (not in the calling thread's
// last-error slot: plk_verify_many_with's workers have none that anybody reads) and *early = 0.

}  // namespace plk
