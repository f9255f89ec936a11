#!/usr/bin/env python3
"""Measures plk_kzg_open_multi_values_dev (kzg_multi_values.hip) on one GPU and writes profiles/kzg_open_multi_values.txt (or the path
given as argv[1]).

At N = 2^20, for (m, p) = (8, 1), (8, 3) with the PLONK-like masks and (32, 8) with pseudo-random masks, two legs alternate in one process:
  (a) the new call on the values, with its four parts (plk_kzg_open_multi_last_ms);
  (b) what a holder of values paid before it: m copies into scratch, m inverse plk_ntt_dev there, then plk_kzg_open_multi_dev, with that
      call's four parts.
Both legs must return the same bytes; the probe stops if they do not.  Protocol: device events on the stream the calls run on, 3 warm-up
calls, the median of 20.  Every opening call blocks, so an event pair around a leg measures it as its caller sees it.  Per-kernel times
need a profiler run of their own: rocprofv3 --kernel-trace --stats -- python tools/kzg_multi_values_probe.py --kernels-only."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "kzg_open_multi_values.txt")
    n = 1 << LOG_N
    ctx = pa.Context(0)
    ctx.srs_generate(n, 0, 42)
    ctx.srs_lagrange_from_powers(LOG_N)
    stream = torch.cuda.Stream()
    lines = ["kzg_multi_values_probe: %s, N = 2^%d, median of %d after %d warm-up calls, device events around each leg, legs alternating"
             % (torch.cuda.get_device_name(0), LOG_N, REPS, WARM)]

    def rand_fr(seed):
        rng = np.random.default_rng(seed)
        a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
        a[:, 3] >>= np.uint64(2)                                  # below r
        return torch.from_numpy(a.view(np.int64)).to("cuda:0")

    values = [rand_fr(i) for i in range(32)]
    scratch = [torch.empty_like(v) for v in values]
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
        d, s = values[:m], scratch[:m]

        def from_values():
            return ctx.kzg_open_multi_values_dev(d, LOG_N, pts, sets, gamma, u, stream=stream)

        def transforms():
            with torch.cuda.stream(stream):
                for a, b in zip(s, d):
                    a.copy_(b)
            for a in s:
                ctx.ntt_dev(a, LOG_N, inverse=True, stream=stream)

        def through_coefficients():
            transforms()
            return ctx.kzg_open_multi_dev(s, n, pts, sets, gamma, u, stream=stream)

        if kernels_only:                                          # for a profiler run: each shape's kernels a few times, nothing else
            for _ in range(WARM):
                from_values()
            continue
        got_a, got_b = from_values(), through_coefficients()
        if any(x.tobytes() != y.tobytes() for x, y in zip(got_a, got_b)):
            raise SystemExit("kzg_multi_values_probe: the two legs disagree at (%d, %d)" % (m, p))
        ctx.set_kernel_timing(True)
        for _ in range(WARM):
            from_values(); through_coefficients()
        rows = {"a": [], "b": [], "ntt": []}
        parts = {"a": [], "b": []}
        for _ in range(REPS):
            rows["a"].append(stamp(from_values))
            parts["a"].append(ctx.kzg_open_multi_last_ms())
            rows["b"].append(stamp(through_coefficients))
            parts["b"].append(ctx.kzg_open_multi_last_ms())
            rows["ntt"].append(stamp(transforms))
        ctx.set_kernel_timing(False)
        med = {k: statistics.median(v) for k, v in rows.items()}
        part = {k: [statistics.median(x[i] for x in v) for i in range(4)] for k, v in parts.items()}
        lines.append("")
        lines.append("(m, p) = (%d, %d), sets %s" % (m, p, " ".join("%x" % x for x in sets)))
        lines.append("  (a) plk_kzg_open_multi_values_dev             %8.3f ms (min %.3f max %.3f): evaluations %.3f, quotient h %.3f, commitment W %.3f, second quotient with W' %.3f"
                     % ((med["a"], min(rows["a"]), max(rows["a"])) + tuple(part["a"])))
        lines.append("  (b) %2d copies + inverse NTTs, then the coefficient route %8.3f ms (min %.3f max %.3f): evaluations %.3f, quotient h %.3f, commitment W %.3f, second quotient with W' %.3f"
                     % ((m, med["b"], min(rows["b"]), max(rows["b"])) + tuple(part["b"])))
        lines.append("      the copies and transforms alone               %8.3f ms (min %.3f max %.3f)" % (med["ntt"], min(rows["ntt"]), max(rows["ntt"])))
        lines.append("  ratio (a) / (b) %.2f; (a)'s median %s (b)'s minimum" % (med["a"] / med["b"], "lies below" if med["a"] < min(rows["b"]) else "does NOT lie below"))
    ctx.close()
    if kernels_only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
