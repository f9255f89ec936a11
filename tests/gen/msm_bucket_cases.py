"""Scalar vectors that sit on the integer thresholds of the MSM's bucket schedule (plonkit_amd/csrc/msm_plan.h, "the bucket schedule").

Pure Python, deterministic, nothing of the library.  A case names the populations of a few (window, coarse bin, fine bucket) cells; a build
(BUILDS) fixes the number of terms n and the window width c; terms(case, build) turns the two into a sparse scalar vector:

  * a term destined for window w and bucket mg carries the scalar (mg + 1) << (c * w).  mg + 1 < 2^(c-1) keeps the signed recoding from
    carrying, and in the top window mg + 1 stays below r >> (c * w), so the scalar is a canonical residue whose only non-zero digit is mg + 1;
  * the occupied positions are spread over 0 .. n-1 by a fixed permutation (k -> k * a + n // 3 mod n, a coprime to n); every other term is
    zero and produces no entry;
  * with the 15-copy table (c = 17, ONE bucket set) a term may carry two windows, s + (s << 17): both entries fall into the same bucket,
    which is how a bin comes to hold more than n entries (`doubled` terms, only where a bin needs them);
  * the expected commitment against the tau = 42 powers is (sum_i s_i 42^i mod r) G: expected_scalar().

Which bucket an entry lands in is exact; the ORDER of a bin's entries is the scatter's (one run per workgroup of the pre-phase, in the order
the workgroups reserved them).  So cases that name a property of a task use bins of at most CHUNK entries (one task: the order does not
matter), and cases with several tasks per bin put all their entries into one bucket.  The "spread" slices cases are for correctness only.
Layout cases (the recoding family, sort_waves_runs) place their terms explicitly instead of by the permutation, because what they name is a
property of the 64-term waves of the pre-phase or of a workgroup's run.

populations() recomputes every bin's bucket populations from the finished scalars (digit by digit, as the recoding would), and
tests/test_msm_bucket_cases_host.py holds that against what the case declares before tests/host/msm_bucket_cases_check.cpp runs the
populations through the rules of msm_plan.h.  matrix() is the list of (case, build) pairs tests/test_gpu_msm_bucket_edges.py runs: every
case in every build whose code it can reach; UNREACHABLE states which pairs are left out and why.
"""
import math
import random

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TAU = 42
CHUNK, THREADS, FINE_BITS, FINE = 16384, 256, 6, 64

# name -> the smallest n that selects the build, and what the build is (tests/test_gpu_msm_bucket_edges.py asserts it through
# Context.msm_last_shape / msm_last_no_inf).  `block`: scalars per workgroup of the pre-phase's scatter (a run of a bin's entries).
BUILDS = {
    "owned":     dict(n=(1 << 15) + 1, c=17, variant=2, bases=False, no_inf=True,  prephase=1, copies=15, nbins=1024, block=1024,
                      families=("mu", "span", "alignment", "owned", "slices", "sort", "recode")),
    "plain":     dict(n=(1 << 16) + 1, c=17, variant=0, bases=False, no_inf=True,  prephase=1, copies=15, nbins=1024, block=1024,
                      families=("mu", "span", "alignment", "slices", "sort", "recode")),
    "plain_inf": dict(n=(1 << 16) + 1, c=17, variant=0, bases=False, no_inf=False, prephase=1, copies=15, nbins=1024, block=1024,
                      families=("span", "alignment", "slices")),
    "bases13":   dict(n=4096,          c=13, variant=2, bases=True,  no_inf=False, prephase=2, copies=1,  nbins=64,   block=16384,
                      families=("mu", "span", "alignment", "owned", "slices", "sort")),
    "bases15":   dict(n=1 << 17,       c=15, variant=0, bases=True,  no_inf=False, prephase=2, copies=1,  nbins=256,  block=16384,
                      families=("span", "slices")),
}
# where a case's bins go: (window, coarse bin), rotated by the case's number so that single-bin cases visit all three.  The last place is the
# TOP window (mg + 1 < r >> (c * w): 49553 at c = 17, 96 at c = 13, 12388 at c = 15).
PLACES = {17: ((0, 0), (7, 1022), (14, 700)), 13: ((0, 0), (7, 62), (19, 0)), 15: ((0, 0), (8, 254), (16, 100))}
# (case, build) pairs of matrix() that a build's family list names but its n cannot hold: a bin of the 4096-term build has at most 4096
# entries (one window per bucket set), so nothing with CHUNK entries in a bin reaches it.
UNREACHABLE = {"bases13": "a bin holds at most n = 4096 entries: no task of CHUNK entries (mu = 64), no second task, no hot three quarters of CHUNK"}


class Case:
    def __init__(self, name, family, bins=None, layout=None, expect=(), extra_n=0, needs=None):
        self.name, self.family, self.bins, self.layout, self.expect, self.extra_n, self.needs = name, family, bins, layout, tuple(expect), extra_n, needs

    def n(self, build):
        return BUILDS[build]["n"] + self.extra_n

    def __repr__(self):
        return "Case(%s)" % self.name


def _windows(c):
    return 254 // c + 1


def _value(c, w, coarse, fine):
    mg = coarse * FINE + fine
    assert mg + 1 < 1 << (c - 1) and (mg + 1) << (c * w) < R_MOD, (c, w, coarse, fine)
    return (mg + 1) << (c * w)


def _stride(n):
    a = int(n * 0.618)
    while math.gcd(a, n) != 1:
        a += 1
    return a


def _spread(total, buckets):
    """`total` entries round-robin over the listed buckets -> {bucket: count}"""
    return {f: total // len(buckets) + (1 if k < total % len(buckets) else 0) for k, f in enumerate(buckets)}


def _bin(*parts):
    out = [0] * FINE
    for part in parts:
        for f, cnt in part.items():
            out[f] += cnt
    return out


# ------------------------------------------------------------------------------------------------ a case -> its terms
def terms(case, build, index=0):
    """[(position, scalar)], position < case.n(build), scalars canonical and non-zero; positions distinct"""
    B = BUILDS[build]
    n, c = case.n(build), B["c"]
    if case.layout is not None:
        out = case.layout(B, n)
    else:
        places = PLACES[c]
        total = sum(sum(b) for b in case.bins)
        values = []
        for j, counts in enumerate(case.bins):
            w, coarse = places[(index + j) % 3]
            spare = sum(counts) - n if len(case.bins) == 1 else 0                   # entries beyond n: as many doubled terms, from the first cells on
            assert spare <= 0 or B["copies"] == 15, (case.name, build, "a bin of more than n entries needs the one bucket set of the 15-copy table")
            w2 = w + 1 if w + 1 < _windows(c) else w - 1
            for f, cnt in enumerate(counts):
                v = _value(c, w, coarse, f)
                d = min(max(spare, 0), cnt // 2)
                spare -= d
                values += [v + _value(c, w2, coarse, f)] * d + [v] * (cnt - 2 * d)
            assert spare <= 0, (case.name, build)
        assert len(values) <= n, (case.name, build, total, n)
        a, b = _stride(n), n // 3
        out = [((k * a + b) % n, v) for k, v in enumerate(values)]
    assert len({p for p, _ in out}) == len(out) and all(0 <= p < n and 0 < v < R_MOD for p, v in out), (case.name, build)
    return out


_POWERS = {}


def expected_scalar(term_list, n):
    """sum_i s_i 42^i mod r"""
    if n not in _POWERS:
        pw, x = [], 1
        for _ in range(n):
            pw.append(x)
            x = x * TAU % R_MOD
        _POWERS[n] = pw
    pw = _POWERS[n]
    return sum(v * pw[p] for p, v in term_list) % R_MOD


def populations(term_list, build):
    """{(bucket set, coarse bin): [count per fine bucket]} recomputed from the scalars, digit by digit"""
    B = BUILDS[build]
    c, sets = B["c"], (1 if B["copies"] == 15 else _windows(B["c"]))
    out, cache = {}, {}
    for _, v in term_list:
        if v not in cache:
            cells = []
            for w in range(_windows(c)):
                d = (v >> (c * w)) & ((1 << c) - 1)
                assert d < 1 << (c - 1), "the digit would carry"
                if d:
                    cells.append((w % sets, (d - 1) >> FINE_BITS, (d - 1) & (FINE - 1)))
            cache[v] = cells
        for s, coarse, f in cache[v]:
            out.setdefault((s, coarse), [0] * FINE)[f] += 1
    return out


def sparse_uniform(n, seed, count=40):
    """a neighbour of the case in a batch: `count` uniform scalars at random positions"""
    rng = random.Random(seed)
    return [(p, rng.randrange(1, R_MOD)) for p in sorted(rng.sample(range(n), count))]


def wave_profile(term_list, n):
    """the 64-term waves of the fused pre-phase: how many hold one repeated non-zero scalar in every live lane (`constant`), only zeros
    (`zero`), or differing scalars (`mixed`); and the same three for the last wave alone, with its live lanes"""
    dense = {}
    for p, v in term_list:
        dense[p] = v
    prof = dict(constant=0, zero=0, mixed=0)
    last = None
    for first in range(0, n, 64):
        live = min(64, n - first)
        vals = {dense.get(first + i, 0) for i in range(live)}
        kind = "mixed" if len(vals) > 1 else ("zero" if vals == {0} else "constant")
        prof[kind] += 1
        last = (kind, live)
    prof["last"] = last
    return prof


# ------------------------------------------------------------------------------------------------ the table
def _span_bin(nc, filler, measured, spoiler=0):
    """bucket 0: `filler` entries in front, bucket 1 the measured one, bucket 2 five entries, bucket 63 the spoiler (or part of the rest),
    the rest spread evenly"""
    rest = list(range(3, 63 if spoiler else 64))
    fixed = {0: filler, 1: measured, 2: 5}
    if spoiler:
        fixed[63] = spoiler
    return _bin(fixed, _spread(nc - sum(fixed.values()), rest))


def _layout_blocks(shift=0, gap_zero=False):
    """64-aligned blocks of 64 equal terms, every block a distinct constant of two digits in ONE coarse bin (windows 3 and 9, bin 77);
    `shift` moves the whole vector by that many terms; gap_zero: only every other block is there (all-zero waves) and the blocks that are
    alternate two scalars term by term (non-constant waves)"""
    def build(B, n):
        out = []
        for blk in range(64):
            base = 64 * (2 * blk if gap_zero else blk) + shift + 4096
            for i in range(64):
                f1, f2 = blk, (blk * 5 + 1 + (i & 1 if gap_zero else 0)) % 64
                out.append((base + i, _value(17, 3, 77, f1) + _value(17, 9, 77, f2)))
        return out
    return build


def _layout_tail(B, n):
    """the last wave (n mod 64 live lanes) holds one constant; the two full waves before it alternate two scalars"""
    out = []
    live = n % 64
    first_last = n - live
    for i in range(live):
        out.append((first_last + i, _value(17, 5, 300, 9)))
    for i in range(128):
        out.append((first_last - 128 + i, _value(17, 5, 300, 10 + (i & 1))))
    return out


def _layout_rounds(B, n):
    """terms 8192 .. 12287, one 4096-term block of the count pass (four rounds of 1024 per thread): wave W of round r is constant when
    W + r is even and alternates two scalars otherwise"""
    out = []
    for r in range(4):
        for W in range(16):
            for i in range(64):
                f = (W + 16 * r) % 64 if (W + r) % 2 == 0 else (W + i) % 64
                out.append((8192 + 1024 * r + 64 * W + i, _value(17, 2, 512, f)))
    return out


def _layout_sort_runs(B, n):
    """four runs of 64 entries of one bin (bucket set 0 / window 0, bin 5), each from a different workgroup of the pre-phase's scatter: three
    of bucket 11 only, one spread over buckets 8 .. 23 (bucket 11 among them).  Whatever order the runs are reserved in, the task's four
    waves are three whole-bucket waves and one mixed wave — provided n holds four scatter blocks (it does not in the 4096-term build, where
    the one workgroup mixes everything)."""
    c, block = B["c"], B["block"]
    step = block if 3 * block + 64 <= n else 64
    out = []
    for run in range(4):
        for i in range(64):
            out.append((run * step + i, _value(c, 0, 5, 11 if run < 3 else 8 + i % 16)))
    return out


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    # ---- mu = ceil(nc / 256): one task of nc entries, round-robin over the 64 buckets
    for nc, mu, idle in ((1, 1, 255), (2, 1, 254), (255, 1, 1), (256, 1, 0), (257, 2, 127), (512, 2, 0), (513, 3, 85)):
        add("mu_nc%d" % nc, "mu", [_bin(_spread(nc, list(range(64))))], expect=[("any", "nc", nc), ("any", "mu", mu), ("any", "idle", idle)])
    # ---- span: a filler bucket in front (2 mu: on a lane boundary, 2 mu - 1: one entry before it), the measured bucket 1, the rest even
    for mu, nc in ((10, 2560), (1, 256), (64, CHUNK)):
        tag = "" if mu == 10 else "_mu%d" % mu
        for name, filler, measured, cls, span in (("span8_on", 2 * mu, 9 * mu, "walked", 8), ("span9_on", 2 * mu, 9 * mu + 1, "folded", 9),
                                                  ("span8_off", 2 * mu - 1, 8 * mu + 1, "walked", 8), ("span9_off", 2 * mu - 1, 8 * mu + 2, "folded", 9)):
            add(name + tag, "span", [_span_bin(nc, filler, measured)], expect=[("any", "mu", mu), ("v0", "bucket", (1, cls, span))])
    add("primary_on", "span", [_span_bin(2560, 20, 10)], expect=[("any", "mu", 10), ("v0", "bucket", (1, "primary", 0))])
    add("span1_off", "span", [_span_bin(2560, 25, 10)], expect=[("any", "mu", 10), ("v0", "bucket", (1, "walked", 1))])
    # ---- alignment: 64 buckets of exactly 4 mu entries — TAIL + 3 HEADs each, every run ends where its lane's piece ends
    even = [40] * 64
    add("aligned_4mu", "alignment", [even], expect=[("any", "mu", 10), ("v0", "all_buckets", ("walked", 3))])
    add("aligned_4mu_shifted", "alignment", [[41] + [40] * 62 + [39]], expect=[("any", "mu", 10), ("v0", "bucket", (0, "walked", 4)), ("v0", "bucket", (63, "walked", 3))])
    # ---- owned (the builds of <= 2^16 terms): the fullest bucket at 8 mu + 24 and one above
    for mu, nc in ((10, 2560), (1, 256)):
        for over in (0, 1):
            add("owned_%s_mu%d" % ("above" if over else "limit", mu), "owned",
                [_bin({0: 8 * mu + 24 + over}, _spread(nc - (8 * mu + 24 + over), list(range(1, 64))))],
                expect=[("any", "mu", mu), ("v2", "owned", not over), ("v2", "max_cnt", 8 * mu + 24 + over)])
    add("owned_sparse_quads", "owned", [[0, 1, 2, 3, 4, 5, 9] * 9 + [0]], expect=[("any", "mu", 1), ("v2", "owned", True), ("any", "counts", (0, 1, 2, 3, 4, 5, 9))])
    add("span8_spoiled", "owned", [_span_bin(2560, 20, 90, spoiler=105)], expect=[("any", "mu", 10), ("v2", "owned", False), ("any", "bucket", (1, "walked", 8)),
                                                                                 ("any", "bucket", (0, "walked", 1)), ("any", "bucket", (2, "primary", 0))])
    add("span9_spoiled", "owned", [_span_bin(2560, 20, 91, spoiler=105)], expect=[("any", "mu", 10), ("v2", "owned", False), ("any", "bucket", (1, "folded", 9)),
                                                                                 ("any", "bucket", (2, "primary", 0))])
    # ---- slices: one bucket of 1, 2, 2, 3, 4 and 5 tasks; then the same counts spread over the bin's 64 buckets (correctness only)
    for count, tasks in ((CHUNK, 1), (CHUNK + 1, 2), (2 * CHUNK, 2), (2 * CHUNK + 1, 3), (4 * CHUNK, 4), (4 * CHUNK + 1, 5)):
        add("slices_one_bucket_%d" % count, "slices", [_bin({37: count})], expect=[("any", "tasks", tasks), ("any", "folded", tasks > 4)])
        add("slices_spread_%d" % count, "slices", [_bin(_spread(count, list(range(64))))], expect=[("any", "tasks", tasks), ("any", "folded", tasks > 4)])
    # ---- the wave shortcut of the sort (wave_hot, msm_accumulate)
    add("sort_hot_three_quarters", "sort", [_bin({21: 3 * CHUNK // 4}, _spread(CHUNK // 4, [f for f in range(64) if f != 21]))],
        expect=[("any", "tasks", 1), ("any", "mu", 64)])
    add("sort_waves_runs", "sort", layout=_layout_sort_runs, expect=[("any", "nc", 256), ("any", "mu", 1), ("any", "runs", (3, 1))])
    # ---- the wave shortcut of the recoding (wave_same_scalar, msm_recode_count / msm_recode_scatter): the fused pre-phase only
    add("recode_blocks", "recode", layout=_layout_blocks(), expect=[("any", "waves", dict(constant=64, mixed=0))])
    add("recode_blocks_shifted", "recode", layout=_layout_blocks(shift=1), expect=[("any", "waves", dict(constant=0, mixed=65))])
    add("recode_tail_1", "recode", layout=_layout_tail, expect=[("any", "waves", dict(constant=1, mixed=2, last=("constant", 1)))])
    add("recode_tail_63", "recode", layout=_layout_tail, extra_n=62, expect=[("any", "waves", dict(constant=1, mixed=2, last=("constant", 63)))])
    add("recode_zero_between", "recode", layout=_layout_blocks(gap_zero=True), expect=[("any", "waves", dict(constant=0, mixed=64))])
    add("recode_rounds", "recode", layout=_layout_rounds, expect=[("any", "waves", dict(constant=32, mixed=32))])
    assert len({c.name for c in out}) == len(out)
    return out


def reachable(case, build):
    """whether the build's n can hold the case: each bin within what n terms can give it"""
    B = BUILDS[build]
    if case.bins is None:
        return True
    counts = [sum(b) for b in case.bins]
    if len(counts) == 1:                                              # (only a case of ONE bin is given doubled terms)
        return counts[0] <= (2 if B["copies"] == 15 else 1) * B["n"]
    return sum(counts) <= B["n"]


def matrix():
    """[(case, number of the case, build)]: every case in every build that runs its family and whose n can hold it"""
    return [(case, k, build) for k, case in enumerate(cases()) for build in BUILDS
            if case.family in BUILDS[build]["families"] and reachable(case, build)]
