"""-m "not gpu": the case table of tests/gen/msm_bucket_cases.py against the bucket schedule's rules (plonkit_amd/csrc/msm_plan.h) —
tests/host/msm_bucket_cases_check.cpp is built as a stand-alone program with AddressSanitizer and UBSan and run directly (it is not loaded
into Python).  The program evaluates the functions the kernels call; this file holds what it prints against what every case's NAME says,
so a threshold that moves fails here, on the CPU, with the name of the case that no longer reaches its boundary — where the GPU table
(tests/test_gpu_msm_bucket_edges.py, which runs gen.matrix()) would go on passing without covering it.

  strike   every (case, build) of the matrix: the populations recomputed from the finished scalars are the declared ones, and the rules
           make of them what the case's `expect` says (mu, tasks, folded, owned, the measured bucket's class and span, the pre-phase's waves)
  cover    per build, every class of COVER is struck by some case; what a build cannot reach is written down in NOT_IN with the reason
  slices   count = 1 .. 5 * CHUNK: non-empty slices that sum to count, none above CHUNK, folded from five tasks on
  spans    random populations: a bucket's entries lie in the pieces of lanes tf .. tl and in no others
  text     the three reduction kernels spell msm_lane_entries out (identical instruction streams: see msm.hip above bucket_span); the
           written-out text is held to the function's here"""
import os
import re
import shutil
import subprocess

import pytest

from tests.gen import msm_bucket_cases as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "msm_bucket_cases_check.cpp")

COVER = ("empty", "primary", "walked_span1", "walked_span8", "folded_span9", "owned_at_limit", "not_owned_one_above",
         "tasks1", "tasks2", "tasks3", "tasks4", "tasks5", "mu1", "mu2", "mu3", "mu64", "idle_lane")
_NO_OWNED_RULE = {"owned_at_limit": "variant 0 has no owned rule", "not_owned_one_above": "variant 0 has no owned rule"}
_NO_MU_FAMILY = {"mu2": "the build's row names no mu family", "mu3": "the build's row names no mu family"}
NOT_IN = {
    "owned": {},
    "plain": dict(_NO_OWNED_RULE),
    "plain_inf": dict(_NO_OWNED_RULE, **_NO_MU_FAMILY),
    "bases13": {k: gen.UNREACHABLE["bases13"] for k in ("tasks2", "tasks3", "tasks4", "tasks5", "mu64")},
    "bases15": dict(_NO_OWNED_RULE, **_NO_MU_FAMILY),
}
# the cases a build's families name but its n cannot hold (gen.reachable), by name: nothing leaves the matrix unseen
LEFT_OUT = {"bases13": {"span8_on_mu64", "span9_on_mu64", "span8_off_mu64", "span9_off_mu64", "sort_hot_three_quarters"} |
                       {"slices_%s_%d" % (k, c) for k in ("one_bucket", "spread") for c in (16384, 16385, 32768, 32769, 65536, 65537)}}


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_bucket_cases") / "msm_bucket_cases_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _clean(r):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


@pytest.fixture(scope="module")
def table(program):
    """{(case name, build): (case, terms, [bin])}, bin = dict(count, tasks, folded, task=[dict(nc, mu, owned, max, idle, short, buckets)]);
    the populations fed to the program are the ones recomputed from the scalars"""
    pairs, text = [], []
    for case, k, build in gen.matrix():
        tl = gen.terms(case, build, k)
        pop = gen.populations(tl, build)
        if case.bins is not None:
            assert sorted(pop.values()) == sorted(case.bins), (case.name, build, "the scalars do not hold the declared populations")
        text.append("case %s %s %d" % (case.name, build, gen.BUILDS[build]["variant"]))
        for key in sorted(pop):
            counts = pop[key]
            exact = sum(counts) <= gen.CHUNK or sum(1 for x in counts if x) == 1
            text.append("bin %d %s" % (exact, " ".join(map(str, counts))))
        text.append("end")
        pairs.append((case, build, tl))
    res = subprocess.run([program, "table"], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=600)
    _clean(res)
    out, cur = {}, None
    it = iter(pairs)
    for line in res.stdout.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "case":
            case, build, tl = next(it)
            assert (w[1], w[2]) == (case.name, build)
            cur = out[(case.name, build)] = (case, tl, [])
        elif w[0] == "bin":
            cur[2].append(dict(count=int(w[3]), tasks=int(w[5]), folded=bool(int(w[7])), task=[]))
        elif w[0] == "task":
            cur[2][int(w[1])]["task"].append(dict(nc=int(w[4]), mu=int(w[6]), owned=int(w[8]), max=int(w[10]), idle=int(w[12]), short=int(w[14]), buckets={}))
        elif w[0] == "bucket":
            cur[2][int(w[1])]["task"][int(w[2])]["buckets"][int(w[3])] = dict(cnt=int(w[4]), cls=w[5], tf=int(w[6]), tl=int(w[7]), span=int(w[8]))
    assert len(out) == len(pairs) and next(it, None) is None
    return out


def _holds(key, want, case, tl, bins, build):
    b0 = bins[0]
    t0 = b0["task"][0]
    if key in ("nc", "mu", "idle"):
        return t0[key] == want, t0[key]
    if key == "max_cnt":
        return t0["max"] == want, t0["max"]
    if key == "owned":
        return t0["owned"] == int(want), t0["owned"]
    if key in ("tasks", "folded"):
        return b0[key] == want and len(b0["task"]) == b0["tasks"], b0[key]
    if key == "bucket":
        f, cls, span = want
        got = t0["buckets"][f]
        return (got["cls"], got["span"]) == (cls, span) and got["tl"] - got["tf"] == span, got
    if key == "all_buckets":
        got = {(b["cls"], b["span"]) for b in t0["buckets"].values()}
        return got == {want}, got
    if key == "counts":
        got = {b["cnt"] for b in t0["buckets"].values()}
        return got == set(want), got
    if key == "runs":                                                  # the runs of 64 entries that the scatter's workgroups hand the one task
        B = gen.BUILDS[build]
        if 3 * B["block"] + 64 > case.n(build):
            return True, None                                          # (one workgroup scatters everything: no run structure to name)
        blocks = {}
        for p, v in tl:
            blocks.setdefault(p // B["block"], []).append((p, v))
        kinds = []
        for blk in blocks.values():
            pop = gen.populations(blk, build)
            counts = next(iter(pop.values()))
            kinds.append(sum(1 for x in counts if x) if len(pop) == 1 and sum(counts) == 64 else -1)
        got = (sum(1 for k in kinds if k == 1), sum(1 for k in kinds if k > 1))
        return got == want and -1 not in kinds, kinds
    assert key == "waves"
    prof = gen.wave_profile(tl, case.n(build))
    return all(prof[k] == v for k, v in want.items()) and prof["zero"] > 0, prof


def test_every_case_strikes_what_its_name_says(table):
    bad = []
    for (name, build), (case, tl, bins) in table.items():
        variant = gen.BUILDS[build]["variant"]
        assert case.expect, name
        for when, key, want in case.expect:
            if when != "any" and when != "v%d" % variant:
                continue
            ok, got = _holds(key, want, case, tl, bins, build)
            if not ok:
                bad.append((name, build, key, want, got))
        # what holds for every case: one bin unless the case says otherwise, no task above CHUNK, the tasks hold the bin
        for b in bins:
            assert sum(t["nc"] for t in b["task"]) == b["count"] and all(0 < t["nc"] <= gen.CHUNK for t in b["task"]), (name, build)
    assert not bad, bad


def test_the_matrix_leaves_out_only_what_is_written_down():
    ran = {(c.name, b) for c, _, b in gen.matrix()}
    for build, B in gen.BUILDS.items():
        named = {c.name for c in gen.cases() if c.family in B["families"]}
        left = {n for n in named if (n, build) not in ran}
        assert left == LEFT_OUT.get(build, set()), (build, left ^ LEFT_OUT.get(build, set()))
    assert len(ran) == len(gen.matrix())
    for c, k, b in gen.matrix():
        assert gen.terms(c, b, k) == gen.terms(c, b, k)                   # deterministic
        if c.family == "recode":
            assert gen.BUILDS[b]["prephase"] == 1


def _struck(table, build):
    hit = {}
    tasks = []                                                         # (mu, fullest bucket, owned, case) of the exact tasks
    for (name, b), (case, tl, bins) in table.items():
        if b != build:
            continue
        for bn in bins:
            hit.setdefault("tasks%d" % bn["tasks"], name)
            for t in bn["task"]:
                hit.setdefault("mu%d" % t["mu"], name)
                if t["idle"]:
                    hit.setdefault("idle_lane", name)
                if t["owned"] >= 0:
                    tasks.append((t["mu"], t["max"], t["owned"], name))
                if t["owned"] == 1:
                    continue                                           # (an owned task's buckets are all whole: they strike no class)
                for bk in t["buckets"].values():
                    label = bk["cls"] if bk["cls"] in ("empty", "primary") else "%s_span%d" % (bk["cls"], bk["span"])
                    hit.setdefault(label, name)
    # the owned rule is struck on both sides when, at ONE mu, a task with a fullest bucket of M entries is owned and one with M + 1 is not
    for mu, mx, owned, name in tasks:
        if owned == 1:
            above = [n for m2, x2, o2, n in tasks if m2 == mu and x2 == mx + 1 and o2 == 0]
            if above:
                hit.setdefault("owned_at_limit", name)
                hit.setdefault("not_owned_one_above", above[0])
    return hit


@pytest.mark.parametrize("build", sorted(gen.BUILDS))
def test_cover(table, build):
    hit = _struck(table, build)
    unstruck = [c for c in COVER if c not in hit and c not in NOT_IN[build]]
    assert not unstruck, (build, unstruck)
    for c, why in NOT_IN[build].items():                               # and what is written off is really out of the build's reach
        assert c in COVER and c not in hit, (build, c, why, hit.get(c))


def test_slices_of_every_count(program):
    res = subprocess.run([program, "slices"], capture_output=True, text=True, timeout=600)
    _clean(res)
    assert "msm_bucket_cases_check slices: ok" in res.stdout, res.stdout + res.stderr


def test_spans_of_random_populations(program):
    res = subprocess.run([program, "spans"], capture_output=True, text=True, timeout=600)
    _clean(res)
    assert "msm_bucket_cases_check spans: ok" in res.stdout, res.stdout + res.stderr


def test_the_reducers_spell_out_the_function():
    """msm_fold_hot, msm_task_reduce and msm_task_reduce_quad write msm_lane_entries' expression out; the two texts are the same"""
    plan = open(os.path.join(ROOT, "plonkit_amd", "csrc", "msm_plan.h")).read()
    m = re.search(r"msm_lane_entries\(uint32_t nc\) \{ return ([^;]+); \}", plan)
    assert m, "msm_lane_entries not found in msm_plan.h"
    body = m.group(1)
    msm = open(os.path.join(ROOT, "plonkit_amd", "csrc", "msm.hip")).read()
    assert msm.count("(nc ? %s : 1)" % body) == 3, body
    assert len(re.findall(r"const uint32_t mu = ", msm)) == 3          # and no fourth derivation of mu in that file
