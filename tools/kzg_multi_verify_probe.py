#!/usr/bin/env python3
"""Measures plk_kzg_verify_multi_many_dev (kzg_multi_verify.hip) on one GPU and writes profiles/kzg_verify_multi_many.txt (or the path
given as the first argument).

  Shapes (3, 3) plonk-like and (32, 8) random sets, 1 / 256 / 4096 valid openings of the tau = 42 key, made by construction
  (tests/gen/kzg_multi_cases.py: commitments and proof points are multiples of G, no prover runs).  Per shape and size:
    - the whole call, and plk_kzg_verify_multi_front_dev alone (the check-and-scalars kernel: the front's share);
    - a loop of plk_kzg_verify_multi over the same openings on 16 host threads (wall clock): the only thing a caller could do before;
  and per size, on the same box in the same process:
    - plk_kzg_verify_many_dev (single-point openings) and plk_pairing_check_many_dev alone: what the call's cost is held against.
Protocol: device events on the stream the calls run on around the call plus a synchronise, 3 warm-up calls, the median of 20.
--device-only leaves the host loops and part 1 out, --sizes=4096 and --shape=32x8 narrow the run: for a run under a kernel-tracing
profiler, which splits the call per kernel."""
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
WARM, REPS = 3, 20
SIZES = (1, 256, 4096)


def main():
    import torch
    import plonkit_amd as pa
    from oracle import oracle_lib as ol
    from tests.gen import kzg_multi_cases as km
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    device_only = "--device-only" in sys.argv
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    sizes = tuple(int(x) for x in opt["sizes"].split(",")) if "sizes" in opt else SIZES
    only_shape = tuple(int(x) for x in opt["shape"].split("x")) if "shape" in opt else None
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "kzg_verify_multi_many.txt")
    ctx = pa.Context(0)
    stream = torch.cuda.Stream()
    g2 = pa.crs42_g2_bytes()
    G = ol.g1_generator()
    lines = ["kzg_multi_verify_probe: %s, median of %d after %d warm-up calls, device events around each call plus a synchronise" %
             (torch.cuda.get_device_name(0), REPS, WARM)]

    def timed(f):
        torch.cuda.synchronize()
        for _ in range(WARM):
            f()
        ms = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream); f(); b.record(stream); b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    def g(k):
        return ol.g1_mul(G, k % R_MOD) if k % R_MOD else np.zeros(8, dtype=np.uint64)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")

    def opening(m, p, sets, seed):
        rng = np.random.default_rng(seed)
        polys = [[int(x) * 0x9e3779b97f4a7c15f39cc0605cedc835 % R_MOD for x in rng.integers(1, 1 << 62, size=5)] for _ in range(m)]
        points = [int(x) * 0x1234567890abcdef1234567 % R_MOD for x in rng.integers(1, 1 << 62, size=p)]
        gamma, u = (int(x) * 0xfedcba9876543210fedcba987 % R_MOD for x in rng.integers(1, 1 << 62, size=2))
        o = km.opening(polys, points, sets, gamma, u)
        return (np.stack([g(km.horner(f, km.TAU)) for f in polys]), np.stack([ol.fr_mont(t) for t in points]),
                np.stack([np.stack([ol.fr_mont(y) for y in row]) for row in o["evals"]]), ol.fr_mont(gamma), ol.fr_mont(u), np.stack([g(o["w"]), g(o["w2"])]))

    single = []                                                      # single-point openings, as tools/kzg_probe.py makes them
    for i in range(16):
        c, zz = [3 + i, 5, 7 + i], 1000 + i
        ft, fz = (c[0] + 42 * c[1] + 42 * 42 * c[2]) % R_MOD, (c[0] + zz * c[1] + zz * zz * c[2]) % R_MOD
        single.append((g(ft), ol.fr_mont(zz), ol.fr_mont(fz), g((ft - fz) * pow(42 - zz, -1, R_MOD))))

    lines.append("")
    lines.append("1. what the call is held against: plk_kzg_verify_many_dev (single-point openings) and plk_pairing_check_many_dev alone")
    for cnt in (() if device_only else sizes):
        sel = [single[i % 16] for i in range(cnt)]
        d = [dev(np.stack([s[j] for s in sel])) for j in range(4)]
        verdict = torch.zeros(cnt + 16, dtype=torch.uint8, device="cuda:0")

        def one_point():
            ctx.kzg_verify_many_dev(d[0], d[1], d[2], d[3], cnt, g2, verdict, stream=stream)
            stream.synchronize()

        def pairing():
            ctx.pairing_check_many_dev(d[0], d[3], cnt, g2, verdict, stream=stream)
            stream.synchronize()
        a, b = timed(one_point), timed(pairing)
        lines.append("  %5d openings: kzg_verify_many_dev %8.2f ms (min %.2f max %.2f)   pairing_check_many_dev %8.2f ms (min %.2f max %.2f)" % ((cnt,) + a + b))

    lines.append("")
    lines.append("2. plk_kzg_verify_multi_many_dev, its front alone, and a loop of plk_kzg_verify_multi on 16 host threads (wall clock)")
    for m, p, sets, name in ((3, 3, km.plonk_like_masks(3), "plonk-like"), (32, 8, km.random_masks(32, 8, 40), "random sets")):
        if only_shape and only_shape != (m, p):
            continue
        base = [opening(m, p, sets, 100 * m + i) for i in range(4)]
        for cnt in sizes:
            sel = [base[i % 4] for i in range(cnt)]
            d = [dev(np.stack([s[j] for s in sel]).reshape(cnt * w, -1)) for j, w in enumerate((m, p, m * p, 1, 1, 2))]
            verdict = torch.zeros(cnt + 16, dtype=torch.uint8, device="cuda:0")
            scalars = torch.zeros(cnt * (m + 3) * 4, dtype=torch.int64, device="cuda:0")

            def whole():
                ctx.kzg_verify_multi_many_dev(m, p, sets, d[0], d[1], d[2], d[3], d[4], d[5], cnt, g2, verdict, stream=stream)
                stream.synchronize()

            def front():
                ctx.kzg_verify_multi_front_dev(m, p, sets, d[0], d[1], d[2], d[3], d[4], d[5], cnt, scalars, verdict, stream=stream)
                stream.synchronize()
            fr = timed(front)
            wh = timed(whole)
            assert verdict[:cnt].cpu().numpy().tolist() == [1] * cnt
            host = "host loop   (skipped)"
            if not device_only:
                def host_one(s):
                    return pa.kzg_verify_multi(s[0], s[1], sets, s[2], s[3], s[4], s[5], g2)
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    ok = list(ex.map(host_one, sel))
                host = "host loop %9.2f ms" % ((time.perf_counter() - t0) * 1e3)
                assert all(ok)
            lines.append("  (%2d, %d) %-11s %5d openings: device %8.2f ms (min %.2f max %.2f)   front alone %7.3f ms (min %.3f max %.3f)   %s" %
                         ((m, p, name, cnt) + wh + fr + (host,)))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
