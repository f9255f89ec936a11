#!/usr/bin/env python3
"""Measures the KZG opening calls (kzg.hip) on one GPU and writes profiles/kzg_open.txt (or the path given as argv[1]).

  1. plk_poly_evaluate_values_at_dev / plk_poly_divide_values_by_linear_dev at 2^16, 2^20, 2^24: time and achieved bytes/s for the
     algorithmic 64 to 96 B per element (f read, the denominators written and read, the quotient written) against the HBM peak.
  2. plk_kzg_open_dev at 2^20 by both routes, and what a caller of the values form had to do before this call existed:
     plk_ntt_dev inverse + plk_poly_divide_by_linear_dev + plk_msm_g1_dev; measured in the same process, alternating.
  3. plk_kzg_verify_many_dev at 1, 256 and 4096 openings against a loop of plk_kzg_verify on 16 host threads.
Protocol: device events on the stream the calls run on, 3 warm-up calls, the median of 20.  Every call here blocks, so an event pair
around a call measures the call as its caller sees it (kernels, the host inversion and the round trips between them); per-kernel times
need a profiler run of their own and are not taken here."""
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                                                # bytes/s, HBM3E spec of the MI355X
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
WARM, REPS = 3, 20


def main():
    import torch
    import plonkit_amd as pa
    from oracle import oracle_lib as ol
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kzg_open.txt")
    ctx = pa.Context(0)
    stream = torch.cuda.Stream()                                 # a stream of its own: the calls, the copies and the events all go there
    lines = ["kzg_probe: %s, median of %d after %d warm-up calls, device events around each blocking call" % (torch.cuda.get_device_name(0), REPS, WARM)]

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

    def rand_fr(n, seed):
        rng = np.random.default_rng(seed)
        a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
        a[:, 3] >>= np.uint64(2)                                  # below r
        return torch.from_numpy(a.view(np.int64)).to("cuda:0")

    z = ol.fr_mont(0x1234567890abcdef1234567890abcdef % R_MOD)
    lines.append("")
    lines.append("1. values helpers (z off the domain); bytes/s for 64 and 96 B per element, share of the %.1f TB/s HBM peak" % (HBM_PEAK / 1e12))
    for log_n in (16, 20, 24):
        n = 1 << log_n
        d_in, d_out = rand_fr(n, log_n), rand_fr(n, 100 + log_n)
        ev = timed(lambda: ctx.poly_evaluate_values_at_dev(d_in, log_n, z, stream=stream))
        dv = timed(lambda: ctx.poly_divide_values_by_linear_dev(d_in, log_n, z, d_out, stream=stream))
        for name, (med, lo, hi) in (("evaluate_values_at", ev), ("divide_values_by_linear", dv)):
            b64, b96 = 64.0 * n / (med * 1e-3), 96.0 * n / (med * 1e-3)
            lines.append("  2^%d %-24s %8.3f ms (min %.3f max %.3f)   %.3f - %.3f TB/s = %.1f - %.1f %% of peak" %
                         (log_n, name, med, lo, hi, b64 / 1e12, b96 / 1e12, 100 * b64 / HBM_PEAK, 100 * b96 / HBM_PEAK))
        del d_in, d_out

    log_n, n = 20, 1 << 20
    ctx.srs_generate(n, 0, 42)
    ctx.srs_lagrange_from_powers(log_n)
    vals = rand_fr(n, 7)
    coeffs = vals.clone()
    torch.cuda.synchronize()
    ctx.ntt_dev(coeffs, log_n, inverse=True)
    ctx.synchronize()
    tmp, q = vals.clone(), vals.clone()

    def parent_route():
        with torch.cuda.stream(stream):
            tmp.copy_(vals)
        ctx.ntt_dev(tmp, log_n, inverse=True, stream=stream)
        ctx.poly_divide_by_linear_dev(tmp, n, z, q, stream=stream)
        ctx.msm_dev(q, n, stream=stream)

    torch.cuda.synchronize()
    a = ctx.kzg_open_dev([vals], n, z, values=True, stream=stream)[1]
    b = ctx.kzg_open_dev([coeffs], n, z, stream=stream)[1]
    assert np.array_equal(a, b)
    rows = {"values": [], "coefficients": [], "parent": []}
    fs = {"values": lambda: ctx.kzg_open_dev([vals], n, z, values=True, stream=stream),
          "coefficients": lambda: ctx.kzg_open_dev([coeffs], n, z, stream=stream), "parent": parent_route}
    for f in fs.values():
        for _ in range(WARM):
            f()
    for _ in range(REPS):                                        # alternating
        for k, f in fs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); f(); e1.record(stream); e1.synchronize()
            rows[k].append(e0.elapsed_time(e1))
    lines.append("")
    lines.append("2. plk_kzg_open_dev, one polynomial of 2^20, alternating in one process (the parent route: copy + plk_ntt_dev inverse + plk_poly_divide_by_linear_dev + plk_msm_g1_dev)")
    for k in ("values", "coefficients", "parent"):
        lines.append("  %-13s %8.3f ms (min %.3f max %.3f)" % (k, statistics.median(rows[k]), min(rows[k]), max(rows[k])))

    lines.append("")
    lines.append("3. plk_kzg_verify_many_dev against a loop of plk_kzg_verify on 16 host threads (wall clock, valid openings of the tau = 42 key)")
    g2 = pa.crs42_g2_bytes()
    G = ol.g1_generator()
    base = []
    for i in range(16):
        c = [3 + i, 5, 7 + i]
        zz = 1000 + i
        ft, fz = (c[0] + 42 * c[1] + 42 * 42 * c[2]) % R_MOD, (c[0] + zz * c[1] + zz * zz * c[2]) % R_MOD
        base.append((ol.g1_mul(G, ft), ol.fr_mont(zz), ol.fr_mont(fz), ol.g1_mul(G, (ft - fz) * pow(42 - zz, -1, R_MOD) % R_MOD)))
    for cnt in (1, 256, 4096):
        sel = [base[i % 16] for i in range(cnt)]
        d = [torch.from_numpy(np.stack([s[j] for s in sel]).view(np.int64)).to("cuda:0") for j in range(4)]
        verdict = torch.zeros(cnt + 16, dtype=torch.uint8, device="cuda:0")

        def dev():
            ctx.kzg_verify_many_dev(d[0], d[1], d[2], d[3], cnt, g2, verdict, stream=stream)
            stream.synchronize()
        med, lo, hi = timed(dev)
        assert verdict[:cnt].cpu().numpy().tolist() == [1] * cnt

        def host_one(s):
            return pa.kzg_verify(s[0][None], s[1], s[2][None], s[3], g2)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            ok = list(ex.map(host_one, sel))
        host_ms = (time.perf_counter() - t0) * 1e3
        assert all(ok)
        lines.append("  %5d openings: device %8.2f ms (min %.2f max %.2f)   host loop %9.2f ms" % (cnt, med, lo, hi, host_ms))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
