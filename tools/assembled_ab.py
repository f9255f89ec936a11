#!/usr/bin/env python3
"""Cost of the assembled-input entry points against plk_prove, on one setup, in one process, interleaved.

Three legs per round, in rotating order: plk_prove (circuit path), plk_prove_assembled_dev (the four columns already in device memory)
and plk_prove_assembled (the four columns in host memory, copied as pageable memory — 4 x 32 MiB at the 2^20 domain against plk_prove's
witness upload).  The columns are those of plk_prove's own proof (prove_trace(0..3), one forward NTT each), so every leg must give the
same bytes; that is checked before timing.  Prints one JSON line: median / p10 / p90 / min / max per leg in milliseconds.

    python tools/assembled_ab.py [--log-n 20] [--lc-terms 0] [--warmup 5] [--proofs 20] [--out FILE]
    python tools/assembled_ab.py --prove-only ...     plk_prove alone (runs on a tree without the assembled entry points: set
                                                      PLK_AB_ROOT to that tree for a before / after A/B of plk_prove itself)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.environ.get("PLK_AB_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median": round(float(np.median(a)), 3), "p10": round(float(np.percentile(a, 10)), 3),
            "p90": round(float(np.percentile(a, 90)), 3), "min": round(float(a[0]), 3), "max": round(float(a[-1]), 3), "n": len(a)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--lc-terms", type=int, default=0, help="0: the pinned-subset chain circuit; 5..64: the dense body")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--proofs", type=int, default=20)
    ap.add_argument("--prove-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import plonkit_amd as pa
    n = 1 << a.log_n
    ctx = pa.Context(0)
    ctx.srs_generate(n, 0, 42)
    circ = pa.Circuit.synthetic_ex(n - 2, lc_terms=a.lc_terms) if a.lc_terms else pa.Circuit.synthetic(n - 2)
    setup = pa.SetupForProver(ctx, circ)
    assert setup.domain_size == n
    want = setup.prove(circ)
    legs = {"plk_prove": lambda: setup.prove(circ)}
    if not a.prove_only:
        cols = [ctx.ntt(ctx.prove_trace(j), a.log_n) for j in range(4)]
        dev = [torch.from_numpy(c.view(np.int64)).to("cuda:0") for c in cols]
        torch.cuda.synchronize()
        legs["plk_prove_assembled_dev"] = lambda: setup.prove_assembled_dev(dev, n)
        legs["plk_prove_assembled"] = lambda: setup.prove_assembled(cols)
    for name, fn in legs.items():
        assert fn() == want, name + ": bytes differ from plk_prove's"
    names = list(legs)
    times = {k: [] for k in names}
    for r in range(a.warmup + a.proofs):
        order = names[r % len(names):] + names[:r % len(names)]
        for k in order:
            t0 = time.perf_counter()
            legs[k]()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                times[k].append(dt)
    out = {"what": "assembled_ab", "log_n": a.log_n, "lc_terms": a.lc_terms, "warmup": a.warmup, "proofs": a.proofs,
           "root": os.environ.get("PLK_AB_ROOT", "tree"), "legs": {k: stats(v) for k, v in times.items()}}
    if "plk_prove_assembled_dev" in out["legs"]:
        p, d = out["legs"]["plk_prove"]["median"], out["legs"]["plk_prove_assembled_dev"]["median"]
        out["dev_vs_prove_pct"] = round(100.0 * (d - p) / p, 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    setup.close(); circ.close(); ctx.close()


if __name__ == "__main__":
    main()
