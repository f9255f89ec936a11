"""The products with lazy Montgomery digits (plonkit_amd/csrc/field29_dev.h: mulw2_lz, sqrw2_lz, mulw2_add_lz, mul2addw_lz) and the two
additions built on them (ec29_dev.h: xyzzw_add_mixed_flag, xyzzw_add_pairs) compiled for the HOST (tests/host/
field29_lazy_digits_check.hip): every form against its masked form at the declared limb bounds, on more than 10^5 random operands and on
operands whose multiplier passes 2^261, every chain shadowed in 128 bits (no column reaches 2^64, result - masked result is 0 or p, both
seen); the additions new against old on more than 10^5 cases each, equal after full reduction.  The same program under the address and
undefined-behaviour sanitizers, as a plain executable.  A form whose worst column does not fit 64 bits must not compile.
No GPU involved (hipcc only compiles)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonkit_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "field29_lazy_digits_check.hip")
FORMS = ("mulw2_lz", "sqrw2_lz", "mulw2_add_lz", "mul2addw_lz")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def _check_output(out):
    for form in FORMS:
        m = re.search(form + r": (\d+) results equal to the masked form's, (\d+) larger by p; largest column ([0-9.]+) \* 2\^64 "
                      r"\(compile-time worst case ([0-9.]+) \* 2\^64, fits: 1\)", out)
        assert m, out
        assert int(m.group(1)) >= 30000 and int(m.group(2)) >= 100, out            # both outcomes seen
        assert float(m.group(3)) <= float(m.group(4)) < 1.0, out                   # no column at 2^64; none above the static worst case
    m = re.search(r"lazy forms: 0 failures in (\d+) calls", out)
    assert m and int(m.group(1)) >= 100000, out
    m = re.search(r"mixed addition: 0 mismatches in (\d+) cases \((\d+) P = \+-Q, (\d+) from a fresh accumulator\)", out)
    assert m and int(m.group(1)) >= 100000 and int(m.group(2)) >= 100 and int(m.group(3)) >= 100, out
    m = re.search(r"full addition: 0 mismatches in (\d+) cases \((\d+) on the hot path, (\d+) doublings in other coordinates, (\d+) results the identity\)", out)
    assert m and int(m.group(1)) >= 100000 and int(m.group(2)) >= 50000 and int(m.group(3)) >= 100 and int(m.group(4)) >= 100, out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the check program twice, compiled side by side: plain, and with the host sanitizers (host code only: no device code, GPU sanitizing off)"""
    d = tmp_path_factory.mktemp("field29_lazy_digits")
    plain, san = str(d / "field29_lazy_digits_check"), str(d / "field29_lazy_digits_check_san")
    jobs = [subprocess.Popen(["hipcc", "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", plain], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(["hipcc", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17",
                              "-I", CSRC, SRC, "-o", san], stderr=subprocess.PIPE, text=True)]
    errs = [j.communicate()[1] for j in jobs]
    assert jobs[0].returncode == 0, errs[0][-4000:]
    return plain, (san if jobs[1].returncode == 0 else None), errs[1]


def test_lazy_digit_forms_and_both_additions_against_the_masked_forms(programs):
    plain, _, _ = programs
    r = subprocess.run([plain], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    _check_output(r.stdout)


def test_the_same_program_under_asan_and_ubsan(programs):
    """a plain executable, nothing preloaded; unsigned wrap-around is defined and is what the limb arithmetic uses"""
    _, san, err = programs
    assert san is not None, "the host sanitizer build of the check program failed:\n" + err[-4000:]
    r = subprocess.run([san], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    _check_output(r.stdout)


def test_a_form_whose_column_does_not_fit_does_not_compile(tmp_path):
    """left limbs at MULW_A_LIMB_MAX fit the masked product (that is its bound) but not eight unmasked digits; with digit 7 alone they fit"""
    body = """#include "field29_dev.h"
using namespace plk;
struct LbMax { static constexpr Limbs9 B = lb_uniform(MULW_A_LIMB_MAX); };
void f(const FqW9 &a, const FqW9 &b, FqW9 &r0, FqW9 &r1) { mulw2_lz<FqW, %s, 0u, LbMax, LbNorm, LbNorm, LbNorm>(a, b, a, b, r0, r1); }
"""
    def compiles(lz):
        src = tmp_path / "fit.hip"
        src.write_text(body % lz)
        r = subprocess.run(["hipcc", "--offload-host-only", "-fsyntax-only", "-std=c++17", "-I", CSRC, str(src)],
                           capture_output=True, text=True, timeout=300)
        return r.returncode == 0, r.stderr
    ok, err = compiles("0u")
    assert ok, err
    ok, err = compiles("0x80u")
    assert ok, err
    ok, err = compiles("LZ_ALL")
    assert not ok and "a column of chain 0 can exceed 64 bits" in err, err


def test_a_masked_form_past_its_left_operand_bound_does_not_compile(tmp_path):
    """the masked forms are the same engine with no digit unmasked and their contracts as declared bounds: mulw2 is this instantiation
    with the left operands at MULW_A_LIMB_MAX, which fits; any 32-bit limb on the left does not"""
    body = """#include "field29_dev.h"
using namespace plk;
struct LbLeft { static constexpr Limbs9 B = lb_uniform(%s); };
void f(const FqW9 &a, const FqW9 &b, FqW9 &r0, FqW9 &r1) { mulw2_lz<FqW, 0u, 0u, LbLeft, LbNorm, LbNorm, LbNorm>(a, b, a, b, r0, r1); }
void g(const FqW9 &a, const FqW9 &b, FqW9 &r0, FqW9 &r1) { mulw2<FqW>(a, b, a, b, r0, r1); }
// the bound the masked wrappers declare for their left operand is the documented constant, limb for limb, and the right one is normalised
constexpr bool all_equal(const Limbs9 &b, uint32_t v) { for (int i = 0; i < 9; i++) if (b.l[i] != v) return false; return true; }
static_assert(all_equal(LbMulwA::B, MULW_A_LIMB_MAX) && all_equal(LbNorm::B, M29), "the masked forms' declared contract");
static_assert(lazy_col_bound(LbMulwA::B, LbNorm::B, LbNone::B, LbNone::B, LbNone::B, FqW::P29, 0).fits, "fits at the bound");
"""
    def compiles(left):
        src = tmp_path / "masked.hip"
        src.write_text(body % left)
        r = subprocess.run(["hipcc", "--offload-host-only", "-fsyntax-only", "-std=c++17", "-I", CSRC, str(src)],
                           capture_output=True, text=True, timeout=300)
        return r.returncode == 0, r.stderr
    ok, err = compiles("MULW_A_LIMB_MAX")
    assert ok, err
    ok, err = compiles("0xffffffffu")
    assert not ok and "a column of chain 0 can exceed 64 bits" in err, err
