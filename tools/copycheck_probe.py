#!/usr/bin/env python3
"""Wall time of the copy-constraint checks (plk_setup_check_permutation, plk_check_copies, plk_check_copies_dev) beside a proof of the same
setup, in one process on one GPU: a plk_circuit_synthetic setup at the 2^log_n domain, the columns of its own proof.
usage: python tools/copycheck_probe.py [log_n=20]   ->  one JSON line (profiles/copycheck_2pow20.txt)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonkit_amd as pa


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append(round(time.perf_counter() - t, 6))
    return r, out


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n = 1 << log_n
    ctx = pa.Context(0)
    ctx.srs_generate(n, 0, 42)
    ctx.srs_lagrange_clear()
    circ = pa.Circuit.synthetic(n - 2)
    setup = pa.SetupForProver(ctx, circ)
    assert setup.domain_size == n
    for _ in range(3):
        setup.prove(circ)
    _, prove_t = timed(lambda: setup.prove(circ), 7)
    cols = [ctx.ntt(ctx.prove_trace(j), log_n) for j in range(4)]
    dev = [torch.from_numpy(c.view(np.int64)).to("cuda:0") for c in cols]
    torch.cuda.synchronize()
    rep_p, perm_t = timed(setup.check_permutation, 6)
    rep_c, copies_t = timed(lambda: setup.check_copies_dev(dev), 6)
    rep_h, host_t = timed(lambda: setup.check_copies(cols), 3)
    assert rep_p.kind == rep_c.kind == rep_h.kind == pa.COPY_OK
    print(json.dumps({"domain": n, "prove_wall_s": sorted(prove_t)[len(prove_t) // 2], "prove_wall_s_all": prove_t, "check_permutation_s": perm_t,
                      "check_copies_dev_s": copies_t, "check_copies_host_s": host_t}))
    setup.close(); circ.close(); ctx.close()


if __name__ == "__main__":
    main()
