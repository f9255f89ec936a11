"""What the caller-supplied transcript costs the calls that do not use it, and what routing Keccak through C callbacks costs against the
built-in transcript.  One GPU, one process, warm; the repository's usual protocol: the parent commit's library and this one alternating,
15 calls each, plk_prove at the 2^12 domain and plk_verify on the golden proof, no transcript set.  Then, on this library alone, plk_prove
at 2^12 with Keccak routed through a C table (tools/transcript_keccak_shim.c) alternating with the built-in, same proof bytes.

    python tools/transcript_ops_ab.py --parent path/to/parent/libplonkit_amd.so > profiles/transcript_ops_ab.txt
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import plonkit_amd as pa  # noqa: E402
from plonkit_amd import _lib  # noqa: E402

SHIM = os.path.join(ROOT, "tools", "tmp_transcript_keccak_shim.so")


def shim():
    if not os.path.exists(SHIM):
        libdir = os.path.dirname(pa.lib_path())
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "transcript_keccak_shim.c"),
                               "-o", SHIM, "-L", libdir, "-lplonkit_amd", "-Wl,-rpath," + libdir])
    return ctypes.CDLL(SHIM)


def report(what, rows, names):
    for name in names:
        r = rows[name]
        print("%-10s %-9s %.3f (%.3f .. %.3f)" % (what, name, statistics.median(r), min(r), max(r)))
    a, b = rows[names[0]], statistics.median(rows[names[1]])
    print("# %s: the median of '%s' %s the min-max spread of '%s'" % (what, names[1], "lies inside" if min(a) <= b <= max(a) else
                                                                       ("is BELOW" if b < min(a) else "is ABOVE"), names[0]))


def prover(lib):
    lib.plk_last_error.restype = ctypes.c_char_p
    h, c, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.plk_create(ctypes.c_int32(0), ctypes.byref(h)) == 0
    assert lib.plk_srs_generate(h, ctypes.c_uint64(1 << 12), ctypes.c_uint64(0), ctypes.c_uint32(42)) == 0
    assert lib.plk_circuit_synthetic(ctypes.c_uint64(4000), ctypes.c_uint64(99), ctypes.byref(c)) == 0
    assert lib.plk_setup_prepare(h, c, ctypes.byref(st)) == 0, lib.plk_last_error()
    buf, ln = ctypes.create_string_buffer(1 << 16), ctypes.c_uint64(0)

    def run():
        assert lib.plk_prove(h, st, c, buf, ctypes.c_uint64(1 << 16), ctypes.byref(ln)) == 0, lib.plk_last_error()
        return buf.raw[:ln.value]
    return run, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--new-first", action="store_true")
    a = ap.parse_args()
    L, P = pa.lib(), ctypes.CDLL(a.parent)
    print("# times in ms: median (min .. max) of %d warm calls per leg, legs alternating in one process" % a.calls)
    gold = [open(os.path.join(ROOT, "tests", "golden", f), "rb").read() for f in ("vk.bin", "proof.bin")]

    def verify_with(lib):
        v = ctypes.c_int32(0)
        assert lib.plk_verify(gold[0], ctypes.c_uint64(len(gold[0])), gold[1], ctypes.c_uint64(len(gold[1])), ctypes.byref(v)) == 0 and v.value == 1

    for lib in (P, L):
        verify_with(lib)
    rows = {"parent": [], "new": []}
    for _ in range(a.calls):
        for name, lib in (("parent", P), ("new", L)):
            t = time.perf_counter(); verify_with(lib); rows[name].append((time.perf_counter() - t) * 1e3)
    report("plk_verify", rows, ("parent", "new"))

    if a.new_first:                                                  # which library's context is created first (an order effect would show here)
        (run_n, h_new), (run_p, _) = prover(L), prover(P)
    else:
        (run_p, _), (run_n, h_new) = prover(P), prover(L)
    order = (("new", run_n), ("parent", run_p)) if a.new_first else (("parent", run_p), ("new", run_n))
    assert order[0][1]() == order[1][1]()                            # warm (the lazily made streams too, in this order), and the same proof bytes
    rows = {"parent": [], "new": []}
    for _ in range(a.calls):
        for name, run in order:
            t = time.perf_counter(); run(); rows[name].append((time.perf_counter() - t) * 1e3)
    report("plk_prove", rows, ("parent", "new"))

    # Keccak through a C table against the built-in, this library, the same context and setup (recorded, no gate)
    ops = _lib._TranscriptOpsStruct()
    shim().shim_keccak_ops(ctypes.byref(ops))
    want = run_n()
    rows = {"builtin": [], "callbacks": []}
    for k in range(a.calls + 1):
        for name, table in (("builtin", None), ("callbacks", ctypes.byref(ops))):
            assert L.plk_ctx_set_transcript(h_new, table) == 0
            t = time.perf_counter(); got = run_n(); dt = (time.perf_counter() - t) * 1e3
            assert got == want
            if k:                                                    # the first pair is the warm-up
                rows[name].append(dt)
    assert L.plk_ctx_set_transcript(h_new, None) == 0
    report("plk_prove", rows, ("builtin", "callbacks"))
    print("done")


if __name__ == "__main__":
    main()
