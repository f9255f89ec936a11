"""plk_verify_many against a loop of plk_verify over the same proofs: per-proof time at count = 1, 16, 256, 4096, the split between host
flattening, copies and the three kernels (HIP events, plk_set_kernel_timing), and the batch size at which the GPU path first beats the host
loop on 16 threads.  One GPU, one process, warm.  With --parent <libplonkit_amd.so of the parent commit>: plk_verify on the golden proof
and a 2^12-domain plk_prove with the two libraries alternating in this process.

    python tools/verify_many_ab.py [--parent path/to/parent/libplonkit_amd.so] > profiles/verify_many_ab.txt
"""
import argparse
import concurrent.futures
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import plonkit_amd as pa  # noqa: E402

DISTINCT = 64                                                        # proofs made; larger batches repeat them (every proof is verified on its own)


def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); f(); ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--sizes", default="1,16,256,4096")
    a = ap.parse_args()
    ctx = pa.Context(0)
    ctx.srs_generate(1 << 10, 0, 42)
    first = pa.Circuit.synthetic_ex(200, 4242, 1)
    setup = pa.SetupForProver(ctx, first)
    vk = setup.verification_key_bytes(pa.crs42_g2_bytes())
    proofs = [setup.prove(pa.Circuit.synthetic_ex(200, 4242, k)) for k in range(1, DISTINCT + 1)]
    key = pa.VerificationKey(ctx, vk, strict_inputs=False)
    L = pa.lib()

    def host_one(p):
        v = ctypes.c_int32(0)
        assert L.plk_verify_ex(vk, ctypes.c_uint64(len(vk)), p, ctypes.c_uint64(len(p)), ctypes.c_uint32(0), ctypes.byref(v)) == 0 and v.value == 1

    pool = concurrent.futures.ThreadPoolExecutor(16)                  # ctypes releases the GIL inside the call
    print("# plk_verify_many vs a loop of plk_verify; times in ms, median of the repetitions (min .. max)")
    print("# count | host 1 thread | host 16 threads | plk_verify_many | per proof: host1 host16 gpu | events: flatten upload mul sum pairing download")
    break_even = None
    for count in [int(x) for x in a.sizes.split(",")]:
        batch = [proofs[i % DISTINCT] for i in range(count)]
        host_n = min(count, 64)                                      # the host loop is linear in count: time 64 and scale
        h1 = med(lambda: [host_one(p) for p in batch[:host_n]], 3)
        h16 = med(lambda: list(pool.map(host_one, batch[:max(host_n, min(count, 256))])), 3)
        n16 = max(host_n, min(count, 256))
        h1_ms, h16_ms = h1[0] * count / host_n, h16[0] * count / n16
        assert key.verify_many(batch).all()                          # warm: arena grown, code loaded
        g = med(lambda: key.verify_many(batch), 5 if count <= 256 else 3)
        ctx.set_kernel_timing(True)
        key.verify_many(batch)
        ev = ctx.verify_many_last_ms()
        ctx.set_kernel_timing(False)
        print("%5d | %10.2f | %10.2f | %9.2f (%.2f .. %.2f) | %8.3f %8.3f %8.3f | %s" % (
            count, h1_ms, h16_ms, g[0], g[1], g[2], h1_ms / count, h16_ms / count, g[0] / count, " ".join("%.2f" % x for x in ev)))
        if break_even is None and g[0] < h16_ms:
            break_even = count
    print("# first measured size at which plk_verify_many beats the 16-thread host loop: %s" % break_even)

    if a.parent:
        P = ctypes.CDLL(a.parent)
        gold = [open(os.path.join(ROOT, "tests", "golden", f), "rb").read() for f in ("vk.bin", "proof.bin")]

        def verify_with(lib):
            v = ctypes.c_int32(0)
            assert lib.plk_verify(gold[0], ctypes.c_uint64(len(gold[0])), gold[1], ctypes.c_uint64(len(gold[1])), ctypes.byref(v)) == 0 and v.value == 1

        print("# plk_verify on the golden proof, the two libraries alternating in this process (ms, median (min .. max) of 15)")
        rows = {"parent": [], "new": []}
        for _ in range(15):
            for name, lib in (("parent", P), ("new", L)):
                t = time.perf_counter(); verify_with(lib); rows[name].append((time.perf_counter() - t) * 1e3)
        for name in ("parent", "new"):
            r = rows[name]
            print("plk_verify %-6s %.3f (%.3f .. %.3f)" % (name, statistics.median(r), min(r), max(r)))

        # a 2^12-domain plk_prove through each library's own C ABI (two contexts on one GPU, one setup each), alternating
        def prover(lib):
            lib.plk_last_error.restype = ctypes.c_char_p
            h, c, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            assert lib.plk_create(ctypes.c_int32(0), ctypes.byref(h)) == 0
            assert lib.plk_srs_generate(h, ctypes.c_uint64(1 << 12), ctypes.c_uint64(0), ctypes.c_uint32(42)) == 0
            assert lib.plk_circuit_synthetic(ctypes.c_uint64(4000), ctypes.c_uint64(99), ctypes.byref(c)) == 0
            assert lib.plk_setup_prepare(h, c, ctypes.byref(st)) == 0, lib.plk_last_error()
            buf, ln = ctypes.create_string_buffer(1 << 16), ctypes.c_uint64(0)

            def run():
                assert lib.plk_prove(h, st, c, buf, ctypes.c_uint64(1 << 16), ctypes.byref(ln)) == 0
                return buf.raw[:ln.value]
            return run
        runs = {"parent": prover(P), "new": prover(L)}
        assert runs["parent"]() == runs["new"]()                     # warm, and the same proof bytes
        rows = {"parent": [], "new": []}
        for _ in range(15):
            for name in ("parent", "new"):
                t = time.perf_counter(); runs[name](); rows[name].append((time.perf_counter() - t) * 1e3)
        print("# plk_prove at the 2^12 domain, same proof bytes, alternating (ms, median (min .. max) of 15)")
        for name in ("parent", "new"):
            r = rows[name]
            print("plk_prove  %-6s %.3f (%.3f .. %.3f)" % (name, statistics.median(r), min(r), max(r)))
    print("done")


if __name__ == "__main__":
    main()
