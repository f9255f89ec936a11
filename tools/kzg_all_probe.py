#!/usr/bin/env python3
"""Measures plk_kzg_open_all_dev (kzg_all.hip) on one GPU and writes profiles/kzg_open_all.txt (or the path given as argv[1]).

  1. The call at 2^12, 2^16 and 2^20: warm (the key's transform kept by the context) and cold (the transform rebuilt inside the call: another
     size is prepared before every cold call, outside the event pair), with the five parts of plk_kzg_open_all_last_ms of the median call.
  2. At 2^12 the loop of N plk_kzg_open_dev calls that a caller needed before this call existed, in the same process, and the ratio.
     (The loop is 4096 blocking calls: 1 warm-up and the median of 5 there, said in the output.)
  3. A reading aid at 2^20: plk_g1_intt_srs_dev at 2^20 times (2 * 21 / 20 + 1) — the two transforms of the pass by stage count — plus the
     measured point-wise kernel, against the warm call.
Protocol as tools/kzg_probe.py: device events on the stream the calls run on, 3 warm-up calls, the median of 20.  The call blocks, so an
event pair around it measures the call as its caller sees it.

`--batch [path]`: plk_kzg_open_all_batch_dev instead, record profiles/kzg_open_all_batch.txt.  Same protocol, the key's transform kept: the
batch call at 2^12 with 1, 4, 16, 64 polynomials and at 2^16 with 1, 4, 16, each with its parts, against the loop of `count`
plk_kzg_open_all_dev calls in the same process, and against the same loop run by ANOTHER BUILD of the library on the same box — the parent
commit's, its path in PLK_KZG_ALL_PROBE_PARENT_LIB — in a child process (`--loops`, started after this process has finished measuring and
closed its context).  Both processes also time plk_g1_intt_srs_dev at 2^20, the stage kernel's own A/B."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
WARM, REPS = 3, 20
LOOP_WARM, LOOP_REPS = 1, 5
PARTS = ("key transform", "scalar NTTs", "point-wise", "inverse 2N", "forward N + affine")
BATCH_CASES = ((12, 1), (12, 4), (12, 16), (12, 64), (16, 1), (16, 4), (16, 16))


def make_timed(stream):
    import torch

    def timed(f, before=None, warm=WARM, reps=REPS, after=None):
        """-> (median, min, max, what `after` returned for the median call)"""
        torch.cuda.synchronize()
        for _ in range(warm):
            if before:
                before()
            f()
        rows = []
        for _ in range(reps):
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream); f(); b.record(stream); b.synchronize()
            rows.append((a.elapsed_time(b), after() if after else None))
        rows.sort(key=lambda r: r[0])
        return rows[len(rows) // 2][0] if len(rows) % 2 else 0.5 * (rows[len(rows) // 2 - 1][0] + rows[len(rows) // 2][0]), rows[0][0], rows[-1][0], rows[len(rows) // 2][1]
    return timed


def rand_fr(n, seed):
    import torch
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)                                      # below r
    return torch.from_numpy(a.view(np.int64)).to("cuda:0")


def loops(ctx, stream, timed):
    """the loop of `count` plk_kzg_open_all_dev calls for every batch case, and plk_g1_intt_srs_dev at 2^20: {name: (median, min, max)}"""
    import torch
    res = {}
    ctx.srs_generate(1 << 20, 0, 42)
    for log_n, count in BATCH_CASES:
        n = 1 << log_n
        polys = rand_fr(count * n, 100 * log_n + count)
        proofs = torch.zeros((count * n, 8), dtype=torch.int64, device="cuda:0")
        ctx.kzg_open_all_prepare(log_n)

        def loop():
            for b in range(count):
                ctx.kzg_open_all_dev(polys[b * n:(b + 1) * n], log_n, proofs[b * n:(b + 1) * n], stream=stream)
        res["loop %d %d" % (log_n, count)] = timed(loop)[:3]
        print("loop 2^%d x %d: %.3f ms" % (log_n, count, res["loop %d %d" % (log_n, count)][0]), file=sys.stderr, flush=True)
        del polys, proofs
    out = torch.zeros((1 << 20, 8), dtype=torch.int64, device="cuda:0")
    res["intt 20"] = timed(lambda: (ctx.g1_intt_srs_dev(20, out, stream=stream), stream.synchronize()))[:3]
    return res


def loops_child():
    """--loops: the library named by PLK_KZG_ALL_PROBE_PARENT_LIB runs loops(); one JSON line on stdout"""
    import torch
    import plonkit_amd as pa
    from plonkit_amd import _lib
    _lib._SO = os.environ["PLK_KZG_ALL_PROBE_PARENT_LIB"]        # before the first call loads the library
    ctx = pa.Context(0)
    ctx.set_kernel_timing(True)                                   # as in the parent process: the same calls under the same settings
    stream = torch.cuda.Stream()
    res = loops(ctx, stream, make_timed(stream))
    ctx.close()
    print("LOOPS " + json.dumps(res), flush=True)


def batch_main(out_path):
    import torch
    import plonkit_amd as pa
    ctx = pa.Context(0)
    ctx.set_kernel_timing(True)
    stream = torch.cuda.Stream()
    timed = make_timed(stream)
    lines = ["kzg_all_probe --batch: %s, median of %d after %d warm-up calls, device events around each blocking call, the key's transform kept" %
             (torch.cuda.get_device_name(0), REPS, WARM)]
    ctx.srs_generate(1 << 20, 0, 42)
    batch = {}
    for log_n, count in BATCH_CASES:
        n = 1 << log_n
        polys = rand_fr(count * n, 100 * log_n + count)
        proofs = torch.zeros((count * n, 8), dtype=torch.int64, device="cuda:0")
        ctx.kzg_open_all_prepare(log_n)
        batch[(log_n, count)] = timed(lambda: ctx.kzg_open_all_batch_dev(polys, count, log_n, proofs, stream=stream), after=ctx.kzg_open_all_last_ms)
        print("batch 2^%d x %d: %.3f ms" % (log_n, count, batch[(log_n, count)][0]), file=sys.stderr, flush=True)
        del polys, proofs
    here = loops(ctx, stream, timed)
    ctx.close()
    parent, lib = None, os.environ.get("PLK_KZG_ALL_PROBE_PARENT_LIB")
    if lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loops"], stdout=subprocess.PIPE, text=True, timeout=900)
        found = [l for l in r.stdout.splitlines() if l.startswith("LOOPS ")]
        assert r.returncode == 0 and found, r.stdout[-2000:]
        parent = json.loads(found[-1][6:])
    lines.append("parent commit's library (PLK_KZG_ALL_PROBE_PARENT_LIB): %s" % ("given, its loops run in a child process after this one's" if lib else "NOT GIVEN: the parent's loops were not measured"))
    lines.append("")
    lines.append("plk_kzg_open_all_batch_dev from coefficients, proofs only; ms, (min max); parts of the median call: " + " | ".join(PARTS))
    table = []
    for log_n, count in BATCH_CASES:
        b, lo = batch[(log_n, count)], here["loop %d %d" % (log_n, count)]
        pl = parent["loop %d %d" % (log_n, count)] if parent else None
        lines.append("  2^%-2d x %-2d batch %9.3f (%.3f %.3f)   loop here %9.3f (%.3f %.3f)   loop parent %s   parts %s" %
                     (log_n, count, b[0], b[1], b[2], lo[0], lo[1], lo[2], "%9.3f (%.3f %.3f)" % tuple(pl) if pl else "not measured", " | ".join("%.3f" % v for v in b[3])))
        table.append((log_n, count, b, lo, pl))
    lines.append("")
    lines.append("plk_g1_intt_srs_dev at 2^20: here %.3f (%.3f %.3f)   parent %s" % (tuple(here["intt 20"]) + ("%.3f (%.3f %.3f)" % tuple(parent["intt 20"]) if parent else "not measured",)))
    if parent:
        b16, p16 = batch[(12, 16)][0], parent["loop 12 16"][0]
        lines.append("condition 1 (the batch of 16 at 2^12 is faster than the parent's loop of 16): %.3f against %.3f ms, %.2f x: %s" % (b16, p16, p16 / b16, "HOLDS" if b16 < p16 else "FAILS"))
        for log_n in (12, 16):
            b1, p1 = batch[(log_n, 1)][0], parent["loop %d 1" % log_n]
            lines.append("condition 2 at 2^%d (count = 1 is not slower than the parent's single call beyond the spread of its 20 samples): %.3f against %.3f ms, "
                         "difference %+.3f, spread (max - min) %.3f: %s" % (log_n, b1, p1[0], b1 - p1[0], p1[2] - p1[1], "HOLDS" if b1 - p1[0] <= p1[2] - p1[1] else "FAILS"))
    lines.append("")
    lines.append("DESIGN.md 4.11e table:")
    lines.append("| size | count | batch call (ms) | per polynomial | loop, this build | loop, parent | parent loop / batch | " + " | ".join(PARTS) + " |")
    lines.append("|---|---|---|---|---|---|---|" + "---|" * len(PARTS))
    for log_n, count, b, lo, pl in table:
        lines.append("| 2^%d | %d | %.3f | %.3f | %.3f | %s | %s | " % (log_n, count, b[0], b[0] / count, lo[0], "%.3f" % pl[0] if pl else "—", "%.2f×" % (pl[0] / b[0]) if pl else "—") +
                     " | ".join("%.3f" % v for v in b[3]) + " |")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    import torch
    import plonkit_amd as pa
    from oracle import oracle_lib as ol
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kzg_open_all.txt")
    sizes = [int(s) for s in os.environ.get("PLK_KZG_ALL_PROBE_SIZES", "12,16,20").split(",")]
    ctx = pa.Context(0)
    ctx.set_kernel_timing(True)
    stream = torch.cuda.Stream()
    timed = make_timed(stream)
    lines = ["kzg_all_probe: %s, median of %d after %d warm-up calls, device events around each blocking call" % (torch.cuda.get_device_name(0), REPS, WARM)]

    ctx.srs_generate(1 << max(sizes), 0, 42)
    lines.append("")
    lines.append("1. plk_kzg_open_all_dev from coefficients, proofs only; parts in ms: " + " | ".join(PARTS))
    table, warm_ms, parts_warm = [], {}, {}
    for log_n in sizes:
        n = 1 << log_n
        coeffs = rand_fr(n, log_n)
        proofs = torch.zeros((n, 8), dtype=torch.int64, device="cuda:0")
        call = lambda: ctx.kzg_open_all_dev(coeffs, log_n, proofs, stream=stream)
        ctx.kzg_open_all_prepare(log_n)
        w = timed(call, after=ctx.kzg_open_all_last_ms)
        c = timed(call, before=lambda: ctx.kzg_open_all_prepare(log_n - 1), after=ctx.kzg_open_all_last_ms)
        warm_ms[log_n], parts_warm[log_n] = w[0], w[3]
        for name, r in (("warm", w), ("cold", c)):
            lines.append("  2^%-2d %s %10.3f ms (min %.3f max %.3f)   parts %s" % (log_n, name, r[0], r[1], r[2], " | ".join("%.3f" % v for v in r[3])))
            table.append((log_n, name, r[0], r[3]))
        if log_n == 12:                                          # the only route there was: one plk_kzg_open_dev per point
            zs = [ol.fr_mont(pow(ol.omega(log_n), i, R_MOD)) for i in range(n)]

            def loop():
                for z in zs:
                    ctx.kzg_open_dev([coeffs], n, z, stream=stream)
            lo = timed(loop, warm=LOOP_WARM, reps=LOOP_REPS)
            lines.append("  2^12 loop of %d plk_kzg_open_dev calls %10.3f ms (min %.3f max %.3f; %d warm-up, median of %d)   = %.1f x the warm call, %.1f x the cold one" %
                         (n, lo[0], lo[1], lo[2], LOOP_WARM, LOOP_REPS, lo[0] / w[0], lo[0] / c[0]))
            assert w[0] < lo[0] and c[0] < lo[0], "the one-pass call is not faster than the loop it replaces"
        del coeffs, proofs

    if 20 in sizes:
        log_n, n = 20, 1 << 20
        out = torch.zeros((n, 8), dtype=torch.int64, device="cuda:0")
        t = timed(lambda: (ctx.g1_intt_srs_dev(log_n, out, stream=stream), stream.synchronize()))
        model = t[0] * (2 * 21 / 20 + 1)
        pw = parts_warm[20][2]
        lines.append("")
        lines.append("3. reading aid at 2^20: plk_g1_intt_srs_dev %.3f ms (min %.3f max %.3f); x (2 * 21 / 20 + 1) = %.3f ms; + point-wise %.3f ms = %.3f ms; warm call %.3f ms (%.2f x)" %
                     (t[0], t[1], t[2], model, pw, model + pw, warm_ms[20], warm_ms[20] / (model + pw)))
    lines.append("")
    lines.append("DESIGN.md 4.11a table:")
    lines.append("| size | state | call (ms) | " + " | ".join(PARTS) + " |")
    lines.append("|---|---|---|" + "---|" * len(PARTS))
    for log_n, name, ms, parts in table:
        lines.append("| 2^%d | %s | %.3f | " % (log_n, name, ms) + " | ".join("%.3f" % v for v in parts) + " |")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--loops"]:
        loops_child()
    elif sys.argv[1:2] == ["--batch"]:
        batch_main(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "kzg_open_all_batch.txt"))
    else:
        main()
