// The Fiat-Shamir transcript of ONE proof as the prover rounds (prover.hip) and the host verifier (verify.cpp) see it: the
// built-in RollingKeccak, or a caller's plk_transcript_ops table (Transcript::new / commit_field_element / get_challenge of
// prove_by_steps::<_, _, T> and verifier::verify::<_, _, T>, src/plonk.rs:160-169,198-204, for a T this library does not have).
// Header only: the host test programs pull verify.cpp in as a single translation unit.
//
// With no table the three calls are RollingKeccak's and status() is PLK_OK for ever.  With one:
//   - the constructor runs begin; the destructor runs end exactly when begin succeeded, whatever path leaves the scope;
//   - the FIRST failure (a callback that returns nonzero, a challenge whose limbs are not below r) is kept with its code and
//     words, no callback but end is called after it, and challenge() returns zero: the user checks status() after every
//     challenge, before anything consumes it.  The words travel with the object, not through set_error, because the batch
//     verifier runs transcripts on worker threads whose last-error slot nobody reads.
#pragma once
#include <string>
#include <string.h>
#include "../../include/plonkit_amd.h"
#include "keccak.h"

namespace plk {

void set_error(const std::string &msg);

class ProofTranscript {
public:
    // The Keccak path stays a few inline instructions in the rounds and the verifiers; everything a table needs is out of line and cold, so that
    // the functions that hold a ProofTranscript compile as they did when they held a RollingKeccak.
    ProofTranscript(const plk_transcript_ops *ops, const char *who) : ops_(ops), who_(who) { if (ops_) begin_foreign(); }
    ~ProofTranscript() { if (begun_) end_foreign(); }
    ProofTranscript(const ProofTranscript &) = delete;
    ProofTranscript &operator=(const ProofTranscript &) = delete;

    void absorb_fr(const host::HFr &v) { if (!ops_) keccak_.absorb_fr(v); else foreign_fr(v); }
    void absorb_g1(const host::HAffine &p) { if (!ops_) keccak_.absorb_g1(p); else foreign_g1(p); }
    host::HFr challenge() { return ops_ ? foreign_challenge() : keccak_.challenge(); }
    int32_t status() const { return rc_; }
    const std::string &message() const { return msg_; }
    // for `PLK_TRY(tr.report())` on the calling thread: the kept failure becomes the call's error
    int32_t report() const { return rc_ == PLK_OK ? PLK_OK : report_failure(); }

private:
#define PLK_TR_COLD __attribute__((noinline, cold))
    PLK_TR_COLD void begin_foreign() {
        const int32_t rc = ops_->begin(ops_->user, &state_);
        if (rc != 0) fail(PLK_ERR_IO, "begin", rc); else begun_ = true;
    }
    PLK_TR_COLD void end_foreign() { ops_->end(ops_->user, state_); }
    PLK_TR_COLD void foreign_fr(const host::HFr &v) {
        if (rc_ != PLK_OK) return;
        plk_fr e; memcpy(e.l, v.l, 32);
        const int32_t rc = ops_->absorb_fr(state_, &e);
        if (rc != 0) fail(PLK_ERR_IO, "absorb_fr", rc);
        calls_++;
    }
    PLK_TR_COLD void foreign_g1(const host::HAffine &p) {
        if (rc_ != PLK_OK) return;
        plk_g1_affine e; memcpy(e.x, p.x.l, 32); memcpy(e.y, p.y.l, 32);      // infinity is (0, 0) here as everywhere in the ABI
        const int32_t rc = ops_->absorb_g1(state_, &e);
        if (rc != 0) fail(PLK_ERR_IO, "absorb_g1", rc);
        calls_++;
    }
    PLK_TR_COLD host::HFr foreign_challenge() {
        host::HFr c = host::HFr::zero();
        if (rc_ != PLK_OK) return c;
        plk_fr e; memset(&e, 0, sizeof e);
        const int32_t rc = ops_->challenge(state_, &e);
        if (rc != 0) { fail(PLK_ERR_IO, "challenge", rc); calls_++; return c; }
        calls_++;
        if (host::HFr::geq_p(e.l)) {
            rc_ = PLK_ERR_ARG;
            msg_ = std::string(who_) + ": the transcript's challenge callback (call " + std::to_string(calls_) +
                   " after begin) gave an element that is not a canonical residue (limbs >= r)";
            return c;
        }
        memcpy(c.l, e.l, 32);
        return c;
    }
    PLK_TR_COLD int32_t report_failure() const { set_error(msg_); return rc_; }
    PLK_TR_COLD void fail(int32_t code, const char *what, int32_t rc) {
        rc_ = code;
        msg_ = std::string(who_) + ": the transcript's " + what + " callback" +
               (begun_ ? " (call " + std::to_string(calls_ + 1) + " after begin)" : "") + " returned " + std::to_string(rc);
    }
#undef PLK_TR_COLD
    const plk_transcript_ops *ops_;
    const char *who_;
    RollingKeccak keccak_;
    void *state_ = nullptr;
    bool begun_ = false;
    uint32_t calls_ = 0;                    // absorb / challenge callbacks made so far (for the words of a failure)
    int32_t rc_ = PLK_OK;
    std::string msg_;
};

// The built-in transcript under ProofTranscript's interface, for code that is instantiated once per kind instead of branching per call (the
// host verifier, verify.cpp): nothing beyond RollingKeccak, a status that is a constant — with it such a function compiles to what it was
// when it declared a RollingKeccak.
struct KeccakTranscript : RollingKeccak {
    KeccakTranscript(const plk_transcript_ops *, const char *) {}
    static constexpr int32_t status() { return PLK_OK; }
};
// hands a transcript's failure, if any, to the caller of the function that owns the transcript, on every return of that function
template <class Tr> struct TranscriptOutcome {
    const Tr &t; int32_t *rc; std::string *msg;
    ~TranscriptOutcome() { if (rc) *rc = t.status(); if (msg && t.status() != PLK_OK) *msg = t.message(); }
};
template <> struct TranscriptOutcome<KeccakTranscript> { const KeccakTranscript &t; int32_t *rc; std::string *msg; };

// what a call that takes a table checks before it uses it
inline bool transcript_ops_complete(const plk_transcript_ops *ops) {
    return ops->begin && ops->absorb_fr && ops->absorb_g1 && ops->challenge && ops->end;
}

}  // namespace plk
