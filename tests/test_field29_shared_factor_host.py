"""The products by a shared factor held in two forms (plonkit_amd/csrc/field29_dev.h: make_tw2_a, mul_tw2, mul_tw2_2, mul_tw2_mulw) and the
mixed addition of msm_accumulate's plain kernel built on them (ec29_dev.h: xyzzw_add_mixed_nflag) compiled for the HOST (tests/host/
field29_shared_factor_check.hip): the forms against mulw as residues on more than 10^5 operands, at the declared limb bounds, with w = 0, 1
and p - 1, every chain shadowed in 128 bits; the addition beside the one it replaces over chains of 250 additions from accumulators at the
coordinate bounds.  The same program under the address and undefined-behaviour sanitizers, as a plain executable.  An instantiation whose
worst column does not fit 64 bits must not compile.  No GPU involved (hipcc only compiles)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonkit_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "field29_shared_factor_check.hip")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def _check_output(out):
    m = re.search(r"make_tw2_a: (\d+) calls; largest column ([0-9.]+) \* 2\^64 \(compile-time worst case ([0-9.]+) \* 2\^64, fits: 1\)", out)
    assert m and int(m.group(1)) >= 100000, out
    assert float(m.group(2)) <= float(m.group(3)) < 1.0, out
    m = re.search(r"mul_tw2: (\d+) calls \((\d+) pairs, (\d+) beside a plain product\), (\d+) lazy results equal to the masked form's, (\d+) larger by p; "
                  r"largest column ([0-9.]+) \* 2\^64 \(compile-time worst case ([0-9.]+) \* 2\^64, fits: 1\)", out)
    assert m and min(int(m.group(i)) for i in (1, 2, 3)) >= 100000, out
    assert int(m.group(4)) >= 100000, out
    assert float(m.group(6)) <= float(m.group(7)) < 1.0, out
    m = re.search(r"shared-factor forms: 0 failures in (\d+) calls", out)
    assert m and int(m.group(1)) >= 400000, out
    m = re.search(r"mixed addition chains: 0 mismatches in (\d+) additions \((\d+) chains of 250, (\d+) from a fresh accumulator\)", out)
    assert m and int(m.group(1)) >= 100000 and int(m.group(1)) == 250 * int(m.group(2)) and int(m.group(3)) >= 40, out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the check program twice, compiled side by side: plain, and with the host sanitizers (host code only: no device code, GPU sanitizing off)"""
    d = tmp_path_factory.mktemp("field29_shared_factor")
    plain, san = str(d / "field29_shared_factor_check"), str(d / "field29_shared_factor_check_san")
    jobs = [subprocess.Popen(["hipcc", "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", plain], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(["hipcc", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17",
                              "-I", CSRC, SRC, "-o", san], stderr=subprocess.PIPE, text=True)]
    errs = [j.communicate()[1] for j in jobs]
    assert jobs[0].returncode == 0, errs[0][-4000:]
    return plain, (san if jobs[1].returncode == 0 else None), errs[1]


def test_shared_factor_forms_against_mulw_and_the_addition_against_the_one_it_replaces(programs):
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


def test_a_tw2_whose_column_does_not_fit_does_not_compile(tmp_path):
    """z with limbs up to 2^31 fits the masked form but not four unmasked digits; any 32-bit limb fits neither"""
    body = """#include "field29_dev.h"
using namespace plk;
struct LbZ { static constexpr Limbs9 B = lb_uniform(%s); };
FqW9 f(const FqW9 &z, const FqW9 &a, const FqW9 &w) { return mul_tw2<FqW, %s, LbZ>(z, a, w); }
static_assert(tw2_col_bound(LbNorm::B, LbTw2A::B, LbNorm::B, FqW::P29, TW2_LZ_ALL).fits && tw2a_col_bound(LbNorm::B, FqW::P29, TW2A_LZ_ALL).fits, "the addition's instantiations");
"""
    def compiles(limb, lz):
        src = tmp_path / "fit.hip"
        src.write_text(body % (limb, lz))
        r = subprocess.run(["hipcc", "--offload-host-only", "-fsyntax-only", "-std=c++17", "-I", CSRC, str(src)],
                           capture_output=True, text=True, timeout=300)
        return r.returncode == 0, r.stderr
    ok, err = compiles("M29", "TW2_LZ_ALL")
    assert ok, err
    ok, err = compiles("(1u << 31)", "0u")
    assert ok, err
    ok, err = compiles("(1u << 31)", "TW2_LZ_ALL")
    assert not ok and "a column of chain 0 can exceed 64 bits" in err, err
    ok, err = compiles("0xffffffffu", "0u")
    assert not ok and "a column of chain 0 can exceed 64 bits" in err, err
