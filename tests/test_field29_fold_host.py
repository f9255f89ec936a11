"""The folded Montgomery digits (plonkit_amd/csrc/field29_dev.h, "THE FOLD": the low digits of a reduction divided out by 2^-29 mod p, no
product per digit) in the forms that the mixed addition of msm_accumulate's plain kernel and the full addition of the 16-lane msm_task_reduce
take (ec29_dev.h: xyzzw_add_mixed_nflag, xyzzw_add_pairs), compiled for the HOST (tests/host/field29_fold_check.hip): every folded form
against mulw as residues on more than 10^5 operands, at the declared limb bounds and with the folded digits' low words chosen (0 and
2^32 - 1), every chain shadowed in 128 bits with the largest column beside the compile-time worst case, folded beside unfolded (the difference
0 or +-p); both additions beside the forms they replace over chains of 250 additions from accumulators at the coordinate bounds.  The same
program under the address and undefined-behaviour sanitizers, as a plain executable.  A fold set with one of the last two digits or with a
gap, and a folded form with a 32-bit-limb operand, must not compile.  No GPU involved (hipcc only compiles)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonkit_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "field29_fold_check.hip")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

FORMS = ["mulw2_add_lz, normalised, addend normalised", "mulw2_add_lz, +-y, addend normalised", "mulw2_add_lz, normalised, addend LbAny",
         "mulw2_add_lz, +-y, addend LbAny", "sqrw2_lz", "mul2addw_lz (Y3)", "make_tw2_a", "mul_tw2_2", "mul_tw2_mulw: tw2 chain", "mul_tw2_mulw: plain chain"]


def _check_output(out):
    for form in FORMS:
        m = re.search(re.escape(form) + r": (\d+) chains; largest column ([0-9.]+) \* 2\^64 \(compile-time worst case ([0-9.]+) \* 2\^64, fits: 1\)", out)
        assert m and int(m.group(1)) >= 30000, (form, out)
        assert float(m.group(2)) <= float(m.group(3)) < 1.0, (form, out)
    m = re.search(r"chosen low words: (\d+) operand pairs built; folded digits with L = 0: (\d+), with L = 2\^32 - 1: (\d+)", out)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) >= 200 and int(m.group(3)) >= 200, out
    m = re.search(r"folded beside unfolded: (\d+) equal integers, (\d+) differing by p", out)
    assert m and int(m.group(1)) + int(m.group(2)) >= 300000, out
    m = re.search(r"folded forms: 0 failures in (\d+) chains", out)
    assert m and int(m.group(1)) >= 300000, out
    m = re.search(r"mixed addition chains: 0 mismatches in (\d+) additions \((\d+) chains of 250, (\d+) from a fresh accumulator", out)
    assert m and int(m.group(1)) >= 100000 and int(m.group(1)) == 250 * int(m.group(2)) and int(m.group(3)) >= 40, out
    m = re.search(r"full addition chains: 0 mismatches in (\d+) additions \((\d+) chains of 250", out)
    assert m and int(m.group(1)) >= 100000 and int(m.group(1)) == 250 * int(m.group(2)), out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the check program twice, compiled side by side: plain, and with the host sanitizers (host code only: no device code, GPU sanitizing off)"""
    d = tmp_path_factory.mktemp("field29_fold")
    plain, san = str(d / "field29_fold_check"), str(d / "field29_fold_check_san")
    jobs = [subprocess.Popen(["hipcc", "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", plain], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(["hipcc", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17",
                              "-I", CSRC, SRC, "-o", san], stderr=subprocess.PIPE, text=True)]
    errs = [j.communicate()[1] for j in jobs]
    assert jobs[0].returncode == 0, errs[0][-4000:]
    return plain, (san if jobs[1].returncode == 0 else None), errs[1]


def test_folded_forms_against_mulw_and_the_additions_against_the_ones_they_replace(programs):
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


BODY = """#include "field29_dev.h"
using namespace plk;
struct LbX { static constexpr Limbs9 B = lb_uniform(%s); };
void f(const FqW9 &a, const FqW9 &b, FqW9 &r0, FqW9 &r1) { mulw2_lz<FqW, LZ_ALL, LZ_ALL, LbX, LbNorm, LbX, LbNorm, %s>(a, b, a, b, r0, r1); }
FqW9 g(const FqW9 &z, const FqW9 &a, const FqW9 &w) { return mul_tw2<FqW, TW2_LZ_ALL, LbNorm, LbTw2A, LbNorm, %s>(z, a, w); }
FqW9 h(const FqW9 &w) { return make_tw2_a<FqW, TW2A_LZ_ALL, LbNorm, %s>(w); }
"""
FOLD_MSG = "a fold set is a prefix of the digits short of the last two"
FIT_MSG = "a column of chain 0 can exceed 64 bits"


def _compiles(tmp_path, limb, f9, f5, f4):
    src = tmp_path / "fold.hip"
    src.write_text(BODY % (limb, f9, f5, f4))
    r = subprocess.run(["hipcc", "--offload-host-only", "-fsyntax-only", "-std=c++17", "-I", CSRC, str(src)], capture_output=True, text=True, timeout=300)
    return r.returncode == 0, r.stderr


def test_the_fold_sets_in_use_compile(tmp_path):
    ok, err = _compiles(tmp_path, "M29", "FOLD9", "FOLD_TW2", "FOLD_TW2A")
    assert ok, err
    ok, err = _compiles(tmp_path, "M29", "0x7u", "0x1u", "0x1u")              # shorter prefixes
    assert ok, err
    ok, err = _compiles(tmp_path, "M29", "0u", "0u", "0u")
    assert ok, err


@pytest.mark.parametrize("f9,f5,f4", [("0xffu", "0u", "0u"), ("0x1ffu", "0u", "0u"), ("0x5u", "0u", "0u"), ("0x7eu", "0u", "0u"),
                                      ("0u", "0xfu", "0u"), ("0u", "0x1fu", "0u"), ("0u", "0x6u", "0u"),
                                      ("0u", "0u", "0x7u"), ("0u", "0u", "0xfu"), ("0u", "0u", "0x2u")])
def test_a_fold_set_with_one_of_the_last_two_digits_or_a_gap_does_not_compile(tmp_path, f9, f5, f4):
    """digit 7 or 8 of nine, 3 or 4 of tw2's five, 2 or 3 of make_tw2_a's four; a set that is not a prefix"""
    ok, err = _compiles(tmp_path, "M29", f9, f5, f4)
    assert not ok and FOLD_MSG in err, err


def test_a_folded_form_with_a_32_bit_limb_operand_does_not_compile(tmp_path):
    ok, err = _compiles(tmp_path, "0xffffffffu", "FOLD9", "FOLD_TW2", "FOLD_TW2A")
    assert not ok and FIT_MSG in err, err
