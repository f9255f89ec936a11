#!/usr/bin/env python3
"""Same-process A/B of the two ways a key file becomes a resident key (and back), for profiles/key_io_ab.txt and DESIGN.md §4:
  load : (a) plk_key_parse + plk_srs_upload   (b) plk_srs_load_key     floor: hipMemcpy of the same bytes from pageable memory
  store: (a) plk_srs_download + plk_key_serialize   (b) plk_srs_store_key
Interleaved pairs on keys made by plk_srs_generate and held as file bytes in host memory; minimum, median and spread per side.
usage: python tools/key_io_ab.py [--logs 20,22,24] [--pairs 5] [--one-load LOG]   (--one-load: a single load, for a profiler)"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401
import plonkit_amd as pa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="20,22,24")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--one-load", type=int, default=0)
    a = ap.parse_args()
    L = pa.lib()
    ctx = pa.Context(0)
    g2 = pa.crs42_g2_bytes()
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)

    def make(log_n):
        n = 1 << log_n
        ctx.srs_generate(n, 0, 42)
        return np.frombuffer(ctx.srs_store_key(g2), dtype=np.uint8).copy(), n

    def load_a(raw, pts, n):
        k = ctypes.c_uint64(0)
        g = ctypes.create_string_buffer(256)
        assert L.plk_key_parse(vp(raw), ctypes.c_uint64(raw.size), vp(pts), ctypes.c_uint64(n), ctypes.byref(k), g) == 0
        assert L.plk_srs_upload(ctx._h, vp(pts), ctypes.c_uint64(n)) == 0

    def load_b(raw):
        ctx.srs_load_key(raw)

    def store_a(pts, out, n):
        ln = ctypes.c_uint64(0)
        assert L.plk_srs_download(ctx._h, ctypes.c_uint64(0), ctypes.c_uint64(n), vp(pts)) == 0
        assert L.plk_key_serialize(vp(pts), ctypes.c_uint64(n), g2, vp(out), ctypes.c_uint64(out.size), ctypes.byref(ln)) == 0

    def store_b(out, n):
        ln = ctypes.c_uint64(0)
        assert L.plk_srs_store_key(ctx._h, ctypes.c_uint32(0), g2, vp(out), ctypes.c_uint64(out.size), ctypes.byref(ln)) == 0

    def timed(f, *args):
        t = time.perf_counter(); f(*args); return time.perf_counter() - t

    def line(name, v):
        v = sorted(v)
        print("  %-44s min %8.2f ms  median %8.2f ms  spread (max - min) %7.2f ms" % (name, 1e3 * v[0], 1e3 * v[len(v) // 2], 1e3 * (v[-1] - v[0])), flush=True)
        return v[0], v[len(v) // 2], v[-1] - v[0]

    if a.one_load:
        raw, n = make(a.one_load)
        load_b(raw)
        print("one load of 2^%d points done" % a.one_load)
        return
    for log_n in [int(x) for x in a.logs.split(",")]:
        raw, n = make(log_n)
        pts, out = np.zeros((n, 8), dtype=np.uint64), np.zeros(raw.size, dtype=np.uint8)
        dev = torch.empty(64 * n, dtype=torch.uint8, device="cuda:0")
        body = torch.from_numpy(raw[8:8 + 64 * n])                       # pageable, unaligned by 8 like the file's body
        load_a(raw, pts, n); load_b(raw); store_a(pts, out, n); store_b(out, n)     # warm: buffers, first-touch of the host pages
        assert bytes(out) == bytes(raw)
        la, lb, fl, sa, sb, fd = [], [], [], [], [], []
        for _ in range(a.pairs):
            la.append(timed(load_a, raw, pts, n))
            lb.append(timed(load_b, raw))
            torch.cuda.synchronize()
            t = time.perf_counter(); dev.copy_(body); torch.cuda.synchronize(); fl.append(time.perf_counter() - t)
            sa.append(timed(store_a, pts, out, n))
            sb.append(timed(store_b, out, n))
            t = time.perf_counter(); body.copy_(dev); torch.cuda.synchronize(); fd.append(time.perf_counter() - t)
        print("2^%d points (%d MiB of file bytes), %d interleaved pairs" % (log_n, raw.size >> 20, a.pairs))
        A = line("load  (a) plk_key_parse + plk_srs_upload", la)
        B = line("load  (b) plk_srs_load_key", lb)
        F = line("load  floor: pageable host-to-device copy", fl)
        print("    (b) / (a) = %.3f (minima)   (b) / floor = %.2f   (a) - (b) = %.2f ms against (a)'s spread %.2f ms" % (B[0] / A[0], B[0] / F[0], 1e3 * (A[0] - B[0]), 1e3 * A[2]))
        A = line("store (a) plk_srs_download + plk_key_serialize", sa)
        B = line("store (b) plk_srs_store_key", sb)
        F = line("store floor: device-to-pageable-host copy", fd)
        print("    (b) / (a) = %.3f (minima)   (b) / floor = %.2f   (a) - (b) = %.2f ms against (a)'s spread %.2f ms" % (B[0] / A[0], B[0] / F[0], 1e3 * (A[0] - B[0]), 1e3 * A[2]), flush=True)
        del dev
    ctx.close()


if __name__ == "__main__":
    main()
