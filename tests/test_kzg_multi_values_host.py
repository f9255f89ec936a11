"""-m "not gpu": builds tests/host/kzg_multi_values_plan_check.cpp, a stand-alone program over kzg_multi_values_plan.h (the host algebra
of the multi-point openings from values) with AddressSanitizer and UBSan, runs it directly (it is not loaded into Python) and holds the
numbers it prints — points on the domain, barycentric scales, (N - 1) / 2, g_j, the values at k_j, sum_i c_i r_i(u) — against the
Python-integer model (tests/gen/kzg_multi_values_cases.py)."""
import os
import random
import shutil
import subprocess

import pytest

from tests.gen import kzg_multi_cases as km
from tests.gen import kzg_multi_values_cases as kv

R = km.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


@pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler on PATH")
def test_the_values_plan_header_under_the_sanitizers_gives_the_models_numbers(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "kzg_multi_values_plan_check.cpp")
    exe = str(tmp_path / "kzg_multi_values_plan_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = random.Random(41)
    cases = []
    for log_n in (1, 3, 5):
        n = 1 << log_n
        for points in kv.directed_points(log_n) + [km.point_cases(log_n, p, seed=p) for p in (1, 3, 8) if p <= n + 2]:
            points = [t for k, t in enumerate(points) if t not in points[:k]]
            p, m = len(points), max(len(points), 3)
            for name, sets in sorted(km.mask_families(m, p, seed=m + p).items()):
                vals = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
                cases.append((log_n, vals, points, sets, rng.randrange(R), rng.choice([0, 1, points[0], kv.domain(log_n)[n - 1], rng.randrange(R)])))
    text = "%d\n" % len(cases)
    want = []
    for log_n, vals, points, sets, gamma, u in cases:
        o = kv.opening(vals, log_n, points, sets, gamma, u)
        text += "%d %d %d %x %x\n%s\n%s\n%s\n%s\n" % (log_n, len(sets), len(points), gamma, u, " ".join("%x" % t for t in points), " ".join("%d" % s for s in sets),
                                                    " ".join("%x" % y for row in o["evals"] for y in row), " ".join("%x" % s for row in o["S"] for s in row))
        mat = km.matrix(points, sets, gamma)
        at = [kv.at_domain_point(t, sum(mat[i][j] * o["S"][i][j] for i in range(len(sets))) % R, o["g"][j], log_n) if o["ks"][j] is not None else 0
              for j, t in enumerate(points)]
        want.append(([int(k is not None) for k in o["ks"]], [kv.eval_scale(t, log_n) for t in points], [kv.rest_sum(log_n)], o["g"], at, [o["v"]]))
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[-1] == ["kzg_multi_values_plan_check:", "ok"]
    assert len(lines) == 6 * len(cases) + 1 and any(any(w[0]) for w in want) and not all(all(w[0]) for w in want)
    for k, w in enumerate(want):
        rows = lines[6 * k:6 * k + 6]
        assert [row[0] for row in rows] == ["on", "scale", "rest", "g", "at", "v"]
        assert [int(x) for x in rows[0][1:]] == w[0], k
        for row, numbers in zip(rows[1:], w[1:]):
            assert [int(x, 16) for x in row[1:]] == numbers, (k, row[0])
