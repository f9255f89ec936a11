// Stand-alone check of plonkit_amd/csrc/prover_math.h (the host scalar algebra of prover rounds 4 and 5).  Built with
// -fsanitize=address,undefined by tests/test_prover_math_host.py and run directly; it is not loaded into Python.
// Every number travels as 64 hex digits of the canonical residue.  One request per line of standard input:
//   point N omega z                                            -> "refused <words>"  |  "ok z_inv zw_inv zN l0z"
//   round N omega alpha beta gamma z v ev0 .. ev9              -> "refused <words>"  |  l0z fz fs, then the 9 linearisation
//                                                                 coefficients, then the 12 + 2 opening coefficients, one line each
//   icoset log_n omega4                                        -> the five constants of the coset iNTT's combine step
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <iostream>
#include <sstream>
#include "../../plonkit_amd/csrc/prover_math.h"

using namespace plk::host;

static HFr parse(const std::string &s) {
    if (s.size() != 64) { fprintf(stderr, "prover_math_check: expected 64 hex digits, got '%s'\n", s.c_str()); exit(2); }
    uint64_t c[4];
    for (int i = 0; i < 4; i++) c[3 - i] = strtoull(s.substr(16 * i, 16).c_str(), nullptr, 16);
    if (HFr::geq_p(c)) { fprintf(stderr, "prover_math_check: not a canonical residue\n"); exit(2); }
    return HFr::from_canonical(c);
}
static std::string show(const HFr &v) {
    uint64_t c[4]; v.to_canonical(c);
    char buf[80];
    snprintf(buf, sizeof buf, "%016llx%016llx%016llx%016llx", (unsigned long long)c[3], (unsigned long long)c[2], (unsigned long long)c[1], (unsigned long long)c[0]);
    return buf;
}
static void line(const HFr *v, int n) { for (int k = 0; k < n; k++) printf("%s%s", k ? " " : "", show(v[k]).c_str()); printf("\n"); }

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string what;
        if (!(in >> what)) continue;
        std::vector<std::string> w;
        for (std::string t; in >> t;) w.push_back(t);
        if (what == "icoset" && w.size() == 2) {
            HFr c[5];
            icoset_constants_from(parse(w[1]), (uint32_t)strtoul(w[0].c_str(), nullptr, 10), c);
            line(c, 5);
            continue;
        }
        if (!((what == "point" && w.size() == 3) || (what == "round" && w.size() == 17))) { fprintf(stderr, "prover_math_check: bad request '%s'\n", text.c_str()); return 2; }
        const uint64_t N = strtoull(w[0].c_str(), nullptr, 10);
        const HFr omega = parse(w[1]);
        ZPoint at;
        if (what == "point") {
            if (const char *refused = challenge_point(parse(w[2]), omega, N, &at)) { printf("refused %s\n", refused); continue; }
            const HFr out[4] = {at.z_inv, at.zw_inv, at.zN, at.l0z};
            printf("ok "); line(out, 4);
            continue;
        }
        const HFr alpha = parse(w[2]), beta = parse(w[3]), gamma = parse(w[4]), v = parse(w[6]);
        if (const char *refused = challenge_point(parse(w[5]), omega, N, &at)) { printf("refused %s\n", refused); continue; }
        Evals ev;
        for (int k = 0; k < 10; k++) ev.v[k] = parse(w[7 + k]);
        ev.v[10] = HFr::zero();                                       // r(z) exists only after these coefficients
        HFr fz, fs, lin[9], at_z[12], at_zw[2];
        permutation_factors(alpha, beta, gamma, at, ev, &fz, &fs);
        linearisation_coefficients(ev, fz, fs, lin);
        opening_coefficients(at.zN, v, at_z, at_zw);
        const HFr head[3] = {at.l0z, fz, fs};
        line(head, 3); line(lin, 9); line(at_z, 12); line(at_zw, 2);
    }
    return 0;
}
