"""-m "not gpu": the scalar front of plk_kzg_verify_multi_many_dev (plonkit_amd/csrc/kzg_multi_verify_dev.h: the checks of one opening and
its count + 3 scalars, what k_kmv_check runs one opening per lane) compiled for the HOST — its functions are __host__ __device__ — by
tests/host/kzg_multi_verify_check.hip, and the plan of a pass (kzg_multi_verify_plan.h).  The cases are written here, to a file, from
tests/gen/kzg_multi_cases.py; every expected scalar is the Python-integer model's (c_values, r_at, z_at), and the program holds the same
cases against km_weights / km_c / km_r_at of kzg_multi_plan.h as well.  The plan's numbers are computed here and compared with what the
program prints.  The same source is built a second time with host AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone executable
(its own main, nothing loaded into Python): every array of a case sits in a heap block of exactly its own length.  No GPU involved."""
import os
import random
import re
import shutil
import subprocess

import pytest

from tests.gen import kzg_multi_cases as km

R = km.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "kzg_multi_verify_check.hip")
GOES_ON, MALFORMED = 1, 2
ALL_ONES = (1 << 256) - 1

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def mont(x):
    """the 256-bit word of x in memory"""
    return (x << 256) % R


def scalars(points, sets, evals, gamma, u):
    """c_0 .. c_{m-1}, -sum c_i r_i(u), -Z_T(u), u from the model; evaluations outside a set are not read"""
    c, z_t = km.c_values(points, sets, gamma, u)
    total = sum(ci * km.r_at(points, mask, row, u) for ci, mask, row in zip(c, sets, evals)) % R
    return c + [(-total) % R, (-z_t) % R, u]


class Case:
    """an opening's scalars as integers below r; `raw` replaces words in memory: {"gamma" | "u" | ("point", j) | ("eval", i, j): word}"""

    def __init__(self, name, points, sets, evals, gamma, u, raw=None, kind=0, state=GOES_ON):
        self.name, self.points, self.sets, self.evals, self.gamma, self.u = name, list(points), list(sets), [list(r) for r in evals], gamma, u
        self.raw, self.kind, self.state = dict(raw or {}), kind, state

    def text(self):
        m, p = len(self.sets), len(self.points)
        words = {"gamma": mont(self.gamma), "u": mont(self.u)}
        words.update({("point", j): mont(t) for j, t in enumerate(self.points)})
        words.update({("eval", i, j): mont(self.evals[i][j]) for i in range(m) for j in range(p)})
        words.update(self.raw)
        want = [mont(x) for x in scalars(self.points, self.sets, self.evals, self.gamma, self.u)] if self.state == GOES_ON else [0] * (m + 3)
        order = ["gamma", "u"] + [("point", j) for j in range(p)] + [("eval", i, j) for i in range(m) for j in range(p)]
        return "%s %d %d %d %d\n%s\n%s\n%s\n" % (self.name, m, p, self.kind, self.state, " ".join("%d" % s for s in self.sets),
                                               " ".join("%064x" % words[k] for k in order), " ".join("%064x" % w for w in want))


def _cases():
    rng = random.Random(20261021)
    rnd = lambda: rng.randrange(R)
    out = []
    for m, p in km.HOST_SHAPES:
        points = km.point_cases(5, p, seed=m)
        for name, sets in sorted(km.mask_families(m, p, seed=m + p).items()):
            out.append(Case("family_%dx%d_%s" % (m, p, name), points, sets, [[rnd() for _ in range(p)] for _ in range(m)], rnd(), rnd()))
    # the plonk-like shape: f_0 at t_0 and t_2, f_1 and f_2 at t_0 and t_1
    pts3, sets3 = [9, 0, km.TAU], km.plonk_like_masks(3)
    assert sets3 == [5, 3, 3]
    ev3 = [[rnd() for _ in range(3)] for _ in range(3)]
    out.append(Case("u_is_a_point_of_every_set", pts3, sets3, ev3, rnd(), pts3[0]))
    c = Case("u_is_a_point_outside_a_set", pts3, sets3, ev3, rnd(), km.TAU)          # t_2: c_1 = c_2 = 0 and Z_T(u) = 0
    want = scalars(c.points, c.sets, c.evals, c.gamma, c.u)
    assert want[1] == want[2] == 0 and want[0] != 0 and want[4] == 0
    out.append(c)
    out.append(Case("u_and_t_are_zero", pts3, sets3, ev3, rnd(), 0))
    out.append(Case("evaluations_0_and_r_minus_1", pts3, sets3, [[0, R - 1, 0], [R - 1, 0, R - 1], [0, 0, R - 1]], R - 1, R - 1))
    out.append(Case("gamma_zero", pts3, sets3, ev3, 0, rnd()))
    out.append(Case("non_residue_outside_a_set", pts3, sets3, ev3, rnd(), rnd(), raw={("eval", 0, 1): ALL_ONES, ("eval", 1, 2): R, ("eval", 2, 2): R + 1}))
    out.append(Case("non_residue_inside_a_set", pts3, sets3, ev3, rnd(), rnd(), raw={("eval", 2, 1): R}, state=MALFORMED))
    out.append(Case("non_residue_inside_the_first_set", pts3, sets3, ev3, rnd(), rnd(), raw={("eval", 0, 0): ALL_ONES}, state=MALFORMED))
    out.append(Case("gamma_is_r", pts3, sets3, ev3, 1, rnd(), raw={"gamma": R}, state=MALFORMED))
    out.append(Case("u_is_r", pts3, sets3, ev3, rnd(), 1, raw={"u": R}, state=MALFORMED))
    out.append(Case("a_point_is_r", pts3, sets3, ev3, rnd(), rnd(), raw={("point", 1): R}, state=MALFORMED))
    out.append(Case("points_on_the_curve", pts3, sets3, ev3, rnd(), rnd(), kind=1))
    out.append(Case("w2_off_the_curve", pts3, sets3, ev3, rnd(), rnd(), kind=2, state=MALFORMED))
    out.append(Case("coordinate_is_q", pts3, sets3, ev3, rnd(), rnd(), kind=3, state=MALFORMED))
    for m, p in ((3, 2), (32, 8)):                                                   # two equal points at every pair of positions
        base = km.point_cases(5, p, seed=7)
        sets = km.all_masks(m, p)
        evals = [[rnd() for _ in range(p)] for _ in range(m)]
        for a in range(p):
            for b in range(a + 1, p):
                pts = list(base)
                pts[b] = pts[a]
                out.append(Case("equal_points_%d_%d_of_%d" % (a, b, p), pts, sets, evals, rnd(), rnd(), state=MALFORMED))
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the check program twice, compiled side by side: plain, and host code only with the host sanitizers (no device code, GPU sanitizing off)"""
    d = tmp_path_factory.mktemp("kzg_multi_verify")
    plain, san = str(d / "kzg_multi_verify_check"), str(d / "kzg_multi_verify_check_san")
    jobs = [subprocess.Popen(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", SRC, "-o", plain], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(["hipcc", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17",
                              SRC, "-o", san], stderr=subprocess.PIPE, text=True)]
    errs = [j.communicate()[1] for j in jobs]
    assert jobs[0].returncode == 0, errs[0][-4000:]
    return plain, (san if jobs[1].returncode == 0 else None), errs[1]


@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    cases = _cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    f = tmp_path_factory.mktemp("kzg_multi_verify_cases") / "cases.txt"
    f.write_text("%d\n" % len(cases) + "".join(c.text() for c in cases))
    return str(f), cases


# ---------------------------------------------------------------------------------------------- the plan, computed here
PASS_MAX, PASS_BYTES, BLOCK = 1 << 16, 64 << 20, 256


def _plan(count, npoints):
    terms, pairs = count + 3, npoints * (npoints - 1) // 2
    per = terms * 32 + terms * 144 + pairs * 32 + 64 + 64 + 2
    pas = min(PASS_MAX, PASS_BYTES // per // BLOCK * BLOCK)
    pad = (pas + 15) // 16 * 16
    sizes = [pas * terms * 32, pas * terms * 144, pas * pairs * 32, pas * 64, pas * 64, pad, pad]
    offsets = [sum(sizes[:k]) for k in range(8)]
    return terms, pairs, per, pas, offsets


def _lane_sum(n, count):
    terms = count + 3
    return sum((lane + 1) * (lane // terms * 64 + lane % terms + 1) for lane in range(n * terms)) % (1 << 64)


def _judge(out, cases):
    lines = out.splitlines()
    want_go, want_bad = sum(c.state == GOES_ON for c in cases), sum(c.state == MALFORMED for c in cases)
    assert lines[-1] == "kzg_multi_verify_check: %d cases, %d go on, %d malformed, 0 mismatches" % (len(cases), want_go, want_bad), out[-4000:]
    assert want_go >= 15 and want_bad >= 30                           # the run cannot pass on one kind alone
    plans = [ln.split() for ln in lines if ln.startswith("plan ")]
    assert len(plans) == len(km.HOST_SHAPES)
    for (m, p), ln in zip(km.HOST_SHAPES, plans):
        terms, pairs, per, pas, offsets = _plan(m, p)
        assert [int(x) for x in ln[1:3]] == [m, p]
        assert [int(ln[4]), int(ln[6]), int(ln[8]), int(ln[10])] == [terms, pairs, per, pas], ln
        assert [int(x) for x in ln[12:20]] == offsets, ln
        assert offsets[-1] <= PASS_BYTES and pas % BLOCK == 0 and 0 < pas <= PASS_MAX
        assert pas == PASS_MAX or (pas + BLOCK) * per > PASS_BYTES    # the largest multiple of 256 that fits
    assert _plan(1, 1)[3] == PASS_MAX and _plan(32, 8)[3] == 9216
    sums = {(int(m.group(1)), int(m.group(2))): int(m.group(3)) for m in re.finditer(r"^lanes (\d+) (\d+) sum (\d+)$", out, re.M)}
    assert sums == {(n, m): _lane_sum(n, m) for m, _ in km.HOST_SHAPES for n in (1, 255, 256, 257)}


def test_the_front_on_the_host_gives_the_models_scalars(programs, listed):
    plain, _, _ = programs
    path, cases = listed
    r = subprocess.run([plain, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _judge(r.stdout, cases)


def test_the_front_under_asan_and_ubsan(programs, listed):
    _, san, err = programs
    assert san is not None, "the host sanitizer build of the check program failed:\n" + err[-4000:]
    path, cases = listed
    r = subprocess.run([san, path], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    _judge(r.stdout, cases)


def test_the_cases_cover_what_the_issue_lists(listed):
    _, cases = listed
    names = {c.name for c in cases}
    for m, p in km.HOST_SHAPES:
        for fam in km.mask_families(m, p):
            assert "family_%dx%d_%s" % (m, p, fam) in names
    assert sum(n.startswith("equal_points_") and n.endswith("_of_2") for n in names) == 1
    assert sum(n.startswith("equal_points_") and n.endswith("_of_8") for n in names) == 28
