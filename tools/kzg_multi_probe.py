#!/usr/bin/env python3
"""Measures plk_kzg_open_multi_dev (kzg_multi.hip) on one GPU and writes profiles/kzg_open_multi.txt (or the path given as argv[1]).

At n = 2^20, for (m, p) = (8, 1), (8, 3) with the PLONK-like masks (all at t_0, two also at t_1, one also at t_2) and (32, 8) with
pseudo-random masks: the call and its four parts (plk_kzg_open_multi_last_ms: evaluations, first quotient, its commitment, second
quotient with its commitment), and beside it what a caller does today for the same openings: one plk_kzg_open_dev per distinct point
over the polynomials opened there (at most 8 per call, so a point with more takes several calls).  Then plk_poly_quotient_multi_dev
alone for the same shapes, with its algorithmic bytes (2 count + 1) x 32 n and the rate they amount to.
Protocol: device events on the stream the calls run on, 3 warm-up calls, the median of 20, the two arms alternating in one process.
Every call here blocks, so an event pair around a call measures the call as its caller sees it; per-kernel times need a profiler run of
their own (rocprofv3 --kernel-trace --stats -- python tools/kzg_multi_probe.py --kernels-only) and are not taken here."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                                                # bytes/s, HBM3E spec of the MI355X
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
WARM, REPS = 3, 20
LOG_N = 20


def main():
    import torch
    import plonkit_amd as pa
    from oracle import oracle_lib as ol
    from tests.gen import kzg_multi_cases as km
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels-only" in sys.argv
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "kzg_open_multi.txt")
    n = 1 << LOG_N
    ctx = pa.Context(0)
    ctx.srs_generate(n, 0, 42)
    stream = torch.cuda.Stream()
    lines = ["kzg_multi_probe: %s, n = 2^%d, median of %d after %d warm-up calls, device events around each blocking call, arms alternating"
             % (torch.cuda.get_device_name(0), LOG_N, REPS, WARM)]

    def rand_fr(seed):
        rng = np.random.default_rng(seed)
        a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
        a[:, 3] >>= np.uint64(2)                                  # below r
        return torch.from_numpy(a.view(np.int64)).to("cuda:0")

    polys = [rand_fr(i) for i in range(32)]
    out = rand_fr(99)
    rng = np.random.default_rng(5)
    pts_int = [int(x) * 0x9e3779b97f4a7c15 % R_MOD for x in rng.integers(2, 1 << 62, size=8)]
    gamma, u = ol.fr_mont(0x1234567890abcdef1234567890abcdef), ol.fr_mont(0xfedcba0987654321fedcba0987654321)
    shapes = [(8, 1, [1] * 8), (8, 3, km.plonk_like_masks(8)), (32, 8, km.random_masks(32, 8, 11))]

    def stamp(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); f(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1)

    for m, p, sets in shapes:
        pts = np.stack([ol.fr_mont(t) for t in pts_int[:p]])
        d = polys[:m]

        def multi():
            return ctx.kzg_open_multi_dev(d, n, pts, sets, gamma, u, stream=stream)

        def per_point():
            for j in range(p):
                here = [d[i] for i in range(m) if (sets[i] >> j) & 1]
                for k in range(0, len(here), 8):
                    ctx.kzg_open_dev(here[k:k + 8], n, pts[j], v=gamma, stream=stream)

        coef = np.stack([np.stack([ol.fr_mont(x) for x in row]) for row in km.matrix(pts_int[:p], sets, 0x1234567890abcdef1234567890abcdef)])

        def quotient():
            ctx.poly_quotient_multi_dev(d, n, pts, coef, out, stream=stream)

        if kernels_only:                                          # for a profiler run: each shape's kernels a few times, nothing else
            for _ in range(WARM):
                quotient()
            continue
        calls_today = sum((sum((s >> j) & 1 for s in sets) + 7) // 8 for j in range(p))
        ctx.set_kernel_timing(True)
        for _ in range(WARM):
            multi(); per_point(); quotient()
        rows = {"multi": [], "per_point": [], "quotient": []}
        parts = []
        for _ in range(REPS):
            rows["multi"].append(stamp(multi))
            parts.append(ctx.kzg_open_multi_last_ms())
            rows["per_point"].append(stamp(per_point))
            rows["quotient"].append(stamp(quotient))
        ctx.set_kernel_timing(False)
        med = {k: statistics.median(v) for k, v in rows.items()}
        part = [statistics.median(x[k] for x in parts) for k in range(4)]
        nbytes = (2 * m + 1) * 32.0 * n
        lines.append("")
        lines.append("(m, p) = (%d, %d), sets %s" % (m, p, " ".join("%x" % s for s in sets)))
        lines.append("  plk_kzg_open_multi_dev            %8.3f ms (min %.3f max %.3f): evaluations %.3f, quotient h %.3f, commitment W %.3f, second quotient with W' %.3f"
                     % (med["multi"], min(rows["multi"]), max(rows["multi"]), part[0], part[1], part[2], part[3]))
        lines.append("  %2d x plk_kzg_open_dev (per point)  %8.3f ms (min %.3f max %.3f)   ratio multi / per point %.2f"
                     % (calls_today, med["per_point"], min(rows["per_point"]), max(rows["per_point"]), med["multi"] / med["per_point"]))
        lines.append("  plk_poly_quotient_multi_dev alone %8.3f ms (min %.3f max %.3f): %.1f MB algorithmic = (2 x %d + 1) x 32 n, %.3f TB/s = %.1f %% of the %.1f TB/s peak (the call, its upload and launches included; kernel times need the profiler run)"
                     % (med["quotient"], min(rows["quotient"]), max(rows["quotient"]), nbytes / 1e6, m, nbytes / (med["quotient"] * 1e-3) / 1e12,
                        100 * nbytes / (med["quotient"] * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
    ctx.close()
    if kernels_only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
