#!/usr/bin/env python3
"""Same-process measurement of the two ways a proving service turns a request (the bytes of a .wtns file) into a proof with the setup
kept, for profiles/wtns_ab.txt and DESIGN.md §4.4b:
  (a) plk_circuit_load(r1cs bytes, wtns bytes) + plk_prove      the only route before plk_prove_wtns: the .r1cs is parsed again per request
  (b) plk_prove_wtns                                            the witness decoded and range-checked by a kernel
  (c) the decode kernel alone, bracketed by events on its stream (the bracket includes the 8-byte verdict memset and its read-back)
and, with --parent-lib, the gate on existing behaviour: plk_prove on a circuit object with the parent commit's library and with this one,
alternating in one process, five warm proofs each.
usage: python tools/wtns_ab.py [--log 20] [--pairs 5] [--parent-lib path/to/parent/libplonkit_amd.so]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import plonkit_amd as pa  # noqa: E402

u64 = ctypes.c_uint64


def series(name, v, unit="ms"):
    s = sorted(v)
    print("  %-58s min %9.3f  median %9.3f  max %9.3f %s   [%s]" % (name, s[0], s[len(s) // 2], s[-1], unit, " ".join("%.3f" % x for x in v)), flush=True)
    return s[0], s[len(s) // 2], s[-1]


class Raw:
    """the few calls of the gate through ctypes alone, so that two builds of the library can be held in one process"""

    def __init__(self, path, log_n):
        self.L = ctypes.CDLL(path)
        self.L.plk_last_error.restype = ctypes.c_char_p
        self.ctx, self.circ, self.setup = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        n = 1 << log_n
        self.ck(self.L.plk_create(ctypes.c_int32(0), ctypes.byref(self.ctx)))
        self.ck(self.L.plk_srs_generate(self.ctx, u64(n), u64(0), ctypes.c_uint32(42)))
        self.ck(self.L.plk_circuit_synthetic(u64(n - 2), u64(0x706c6f6e6b6974), ctypes.byref(self.circ)))
        self.ck(self.L.plk_setup_prepare(self.ctx, self.circ, ctypes.byref(self.setup)))
        self.buf, self.len = ctypes.create_string_buffer(1 << 16), u64(0)

    def ck(self, rc):
        if rc != 0:
            raise RuntimeError("status %d: %s" % (rc, self.L.plk_last_error().decode()))

    def prove(self):
        t = time.perf_counter()
        self.ck(self.L.plk_prove(self.ctx, self.setup, self.circ, self.buf, u64(len(self.buf)), ctypes.byref(self.len)))
        return 1e3 * (time.perf_counter() - t), self.buf.raw[:self.len.value]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    log_n, n = a.log, 1 << a.log
    ctx = pa.Context(0)
    ctx.srs_generate(n, 0, 42)
    ctx.srs_precompute()
    base = pa.Circuit.synthetic(n - 2)                                  # the pinned-subset circuit of the bench
    r1cs = base.export("r1cs")
    setup = pa.SetupForProver(ctx, base)
    requests = []
    for ws in range(1, a.pairs + 2):                                    # a witness per request, the same R1CS
        c = pa.Circuit.synthetic_ex(n - 2, witness_seed=ws)
        requests.append(c.export("wtns"))
        c.close()
    print("2^%d domain, pinned-subset circuit: %.1f MiB of .r1cs, %.1f MiB of .wtns per request, %d requests per route, interleaved"
          % (log_n, len(r1cs) / 2**20, len(requests[0]) / 2**20, a.pairs), flush=True)

    def route_a(wt):
        t = time.perf_counter()
        c = pa.Circuit(r1cs, False, wt, False)
        t_load = time.perf_counter()
        proof = setup.prove(c)
        t_end = time.perf_counter()
        w0 = setup.timings_ms()["witness"]
        c.close()
        return 1e3 * (t_end - t), 1e3 * (t_load - t), w0, proof

    def route_b(wt):
        t = time.perf_counter()
        proof = setup.prove_wtns(wt)
        t_end = time.perf_counter()
        return 1e3 * (t_end - t), setup.timings_ms()["witness"], proof

    assert route_a(requests[-1])[3] == route_b(requests[-1])[2]          # warm: workspace, staging arena, cached extensions
    wa, la, fa, wb, fb = [], [], [], [], []
    for wt in requests[:a.pairs]:
        ra = route_a(wt)
        rb = route_b(wt)
        assert ra[3] == rb[2], "the two routes gave different proofs"
        wa.append(ra[0]); la.append(ra[1]); fa.append(ra[2]); wb.append(rb[0]); fb.append(rb[1])
    A = series("(a) Circuit(r1cs, wtns) + prove: wall per request", wa)
    series("(a)   of which plk_circuit_load", la)
    series("(a)   plk_prove_timings[0]", fa)
    B = series("(b) prove_wtns: wall per request", wb)
    series("(b)   plk_prove_timings[0]", fb)
    print("    (a) / (b) = %.2f (medians), %.2f (minima)" % (A[1] / B[1], A[0] / B[0]), flush=True)

    # (c) the decode kernel alone
    wt = requests[0]
    cnt = (len(wt) - 76) // 32
    src = torch.from_numpy(np.frombuffer(bytearray(wt[76:]), dtype=np.uint8)).to("cuda:0")
    dst = torch.empty((cnt, 4), dtype=torch.int64, device="cuda:0")
    s = torch.cuda.Stream()
    ctx.fr_decode_dev(src, cnt, dst, stream=s)
    ks = []
    for _ in range(a.pairs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        ctx.fr_decode_dev(src, cnt, dst, stream=s)
        e1.record(s)
        e1.synchronize()
        ks.append(e0.elapsed_time(e1))
    K = series("(c) fr_decode_kernel, %d elements (events on its stream)" % cnt, ks)
    print("    %.3f ns per element at the minimum; %.1f GB/s of bytes read + written" % (1e6 * K[0] / cnt, 64 * cnt / (K[0] * 1e-3) / 1e9), flush=True)
    setup.close()
    base.close()
    ctx.close()

    if a.parent_lib:
        print("gate: plk_prove on a circuit object, parent library and this one alternating, %d warm proofs each" % a.pairs, flush=True)
        old, new = Raw(os.path.abspath(a.parent_lib), log_n), Raw(pa.lib_path(), log_n)
        for _ in range(3):                                               # warm both: tables, workspaces, page-locked witness
            po_, pn_ = old.prove()[1], new.prove()[1]
        assert po_ == pn_, "the parent's proof bytes differ"
        to, tn = [], []
        for _ in range(a.pairs):
            to.append(old.prove()[0])
            tn.append(new.prove()[0])
        O = series("parent  plk_prove wall", to)
        N = series("this    plk_prove wall", tn)
        ok = N[1] <= O[2]
        print("    this median %.3f ms against the parent's min-max [%.3f, %.3f] ms: %s (same proof bytes)"
              % (N[1], O[0], O[2], "not slower" if ok else "SLOWER THAN THE PARENT'S WHOLE SPREAD"), flush=True)
        return 0 if ok else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
