"""plk_verify_many_packed (front end in a kernel) against plk_verify_many (front end on 16 host threads) on the same proofs: the two calls
alternate, 15 each, at 256, 4096 and 65536 proofs; median and range per call, and the per-stage columns of plk_verify_many_last_ms from a
timed run of their own (slot [0] is the host flattening for plk_verify_many and the front kernel for the packed call).  The condition for
keeping the packed call is printed as it is evaluated: its median at the largest size must lie below plk_verify_many's by more than
plk_verify_many's own min-max spread in this run.  One GPU, one process, warm.  With --parent <libplonkit_amd.so of the parent commit>:
plk_verify on the golden proof and plk_verify_many at 256 proofs with the two libraries alternating in this process.

    python tools/verify_front_ab.py [--parent path/to/parent/libplonkit_amd.so] > profiles/verify_front_ab.txt
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import plonkit_amd as pa  # noqa: E402

DISTINCT = 64                                                        # proofs made; larger batches repeat them (every proof is verified on its own)
CALLS = 15


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def alternate(fns, calls=CALLS):
    """name -> list of wall-clock ms, the functions taking turns"""
    rows = {name: [] for name, _ in fns}
    for _ in range(calls):
        for name, f in fns:
            t = time.perf_counter(); f(); rows[name].append((time.perf_counter() - t) * 1e3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--sizes", default="256,4096,65536")
    ap.add_argument("--calls", type=int, default=CALLS)
    a = ap.parse_args()
    ctx = pa.Context(0)
    ctx.srs_generate(1 << 10, 0, 42)
    first = pa.Circuit.synthetic_ex(200, 4242, 1)
    setup = pa.SetupForProver(ctx, first)
    vk = setup.verification_key_bytes(pa.crs42_g2_bytes())
    proofs = [setup.prove(pa.Circuit.synthetic_ex(200, 4242, k)) for k in range(1, DISTINCT + 1)]
    key = pa.VerificationKey(ctx, vk, strict_inputs=False)
    L = pa.lib()

    print("# plk_verify_many (host front end) vs plk_verify_many_packed (front kernel), alternating, %d calls each; ms, median (min .. max)" % a.calls)
    print("# proofs of %d bytes; events: front upload mul sum+affine pairing download (front = host wall clock for plk_verify_many, the kernel for packed)" % len(proofs[0]))
    print("# count | plk_verify_many | plk_verify_many_packed | events many | events packed")
    wins, last = None, None
    for count in [int(x) for x in a.sizes.split(",")]:
        batch = [proofs[i % DISTINCT] for i in range(count)]
        blob = b"".join(batch)
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in batch], dtype=np.uint64)
        n = len(batch)
        ptrs = (ctypes.c_char_p * n)(*batch)
        lens = (ctypes.c_uint64 * n)(*[len(p) for p in batch])
        verdict = np.zeros(n, dtype=np.uint8)
        fb = ctypes.c_uint64(0)

        # both through the C ABI with the arguments marshalled once: what is timed is the call
        def many():
            assert L.plk_verify_many(ctx._h, key._h, ptrs, lens, ctypes.c_uint64(n), verdict.ctypes.data_as(ctypes.c_void_p), ctypes.byref(fb)) == 0

        def packed():
            assert L.plk_verify_many_packed(ctx._h, key._h, blob, ctypes.c_uint64(len(blob)), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                                            verdict.ctypes.data_as(ctypes.c_void_p), ctypes.byref(fb)) == 0
        for f in (many, packed):                                      # warm: arena grown, code loaded, and every verdict "valid"
            verdict[:] = 0
            f()
            assert verdict.all() and fb.value == 2 ** 64 - 1
        rows = alternate([("many", many), ("packed", packed)], a.calls)
        ev = {}
        ctx.set_kernel_timing(True)
        for name, f in (("many", many), ("packed", packed)):
            f()
            ev[name] = ctx.verify_many_last_ms()
        ctx.set_kernel_timing(False)
        m, p = stats(rows["many"]), stats(rows["packed"])
        print("%6d | %9.2f (%.2f .. %.2f) | %9.2f (%.2f .. %.2f) | %s | %s" % (
            count, m[0], m[1], m[2], p[0], p[1], p[2], " ".join("%.2f" % x for x in ev["many"]), " ".join("%.2f" % x for x in ev["packed"])))
        if wins is None and p[0] < m[0]:
            wins = count
        last = (count, m, p)
    count, m, p = last
    spread = m[2] - m[1]
    print("# condition at %d proofs: packed median %.2f < plk_verify_many median %.2f - its spread %.2f = %.2f : %s" % (
        count, p[0], m[0], spread, m[0] - spread, "HOLDS" if p[0] < m[0] - spread else "DOES NOT HOLD"))
    print("# smallest measured count at which the packed call's median is the lower one: %s" % wins)

    if a.parent:
        P = ctypes.CDLL(a.parent)
        gold = [open(os.path.join(ROOT, "tests", "golden", f), "rb").read() for f in ("vk.bin", "proof.bin")]

        def verify_with(lib):
            def run():
                v = ctypes.c_int32(0)
                assert lib.plk_verify(gold[0], ctypes.c_uint64(len(gold[0])), gold[1], ctypes.c_uint64(len(gold[1])), ctypes.byref(v)) == 0 and v.value == 1
            return run

        def many_with(lib):                                           # a context and a resident key of the library's own
            lib.plk_last_error.restype = ctypes.c_char_p
            h, k = ctypes.c_void_p(), ctypes.c_void_p()
            assert lib.plk_create(ctypes.c_int32(0), ctypes.byref(h)) == 0
            assert lib.plk_vk_load(h, vk, ctypes.c_uint64(len(vk)), ctypes.c_uint32(0), ctypes.byref(k)) == 0, lib.plk_last_error()
            batch = [proofs[i % DISTINCT] for i in range(256)]
            ptrs = (ctypes.c_char_p * 256)(*batch)
            lens = (ctypes.c_uint64 * 256)(*[len(p) for p in batch])
            verdict = np.zeros(256, dtype=np.uint8)
            fb = ctypes.c_uint64(0)

            def run():
                assert lib.plk_verify_many(h, k, ptrs, lens, ctypes.c_uint64(256), verdict.ctypes.data_as(ctypes.c_void_p), ctypes.byref(fb)) == 0 and verdict.all()
            return run
        for title, make in (("plk_verify on the golden proof", verify_with), ("plk_verify_many at 256 proofs", many_with)):
            fns = [("parent", make(P)), ("new", make(L))]
            for _, f in fns:
                f()
            rows = alternate(fns, a.calls)
            print("# %s, the parent commit's library and this one alternating in this process (ms, median (min .. max) of %d)" % (title, a.calls))
            for name in ("parent", "new"):
                s = stats(rows[name])
                print("%-8s %.3f (%.3f .. %.3f)" % (name, s[0], s[1], s[2]))
            sp, sn = stats(rows["parent"]), stats(rows["new"])
            print("# new median inside the parent's spread: %s" % ("yes" if sp[1] <= sn[0] <= sp[2] else "NO"))
    print("done")


if __name__ == "__main__":
    main()
