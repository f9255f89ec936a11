// AddressSanitizer + UndefinedBehaviorSanitizer build of the host verifier under a caller's transcript: the host sources behind
// plk_verify_with / plk_verify_terms_with (hostapi.cpp, pairing.cpp, verify.cpp with transcript_ops.h) in one translation unit, linked with
// tests/host/transcript_ops.c (-DTRANSCRIPT_OPS_HOST_ONLY), whose main runs the host half: every begin there allocates and every end frees,
// so a missing end is a leak and a doubled one a double free.  gcc, no HIP, no GPU, no preloaded runtime.  Driver: tests/test_transcript_ops_c.py.
#include "../../plonkit_amd/csrc/hostapi.cpp"
#include "../../plonkit_amd/csrc/pairing.cpp"
#include "../../plonkit_amd/csrc/verify.cpp"

namespace plk {
static thread_local std::string g_err;
void set_error(const std::string &m) { g_err = m; }
}
extern "C" const char *plk_last_error(void) { return plk::g_err.c_str(); }
