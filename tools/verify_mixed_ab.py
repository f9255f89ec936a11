"""plk_verify_mixed_packed (one call over four verification keys) against the way without it, four plk_verify_many_packed calls, on the same
proofs: the two ways alternate, 15 rounds each, at 4 x 64, 4 x 1024 and 4 x 16384 proofs interleaved by key; once with four keys of ONE G2
pair (the set holds one line table: the single-key pairing kernel) and once with four keys of FOUR G2 pairs (vm_pairing_mixed_kernel,
per-lane line loads).  Median and range per way, and the per-stage columns of plk_verify_many_last_ms of the mixed call from a timed run of
its own.  The condition for keeping the feature is printed as it is evaluated, at 4 x 1024 proofs of one G2 pair: the mixed call's median
must lie below the sum of the four calls' medians by more than the min-max spread of that sum over the rounds.  The keys and proofs are
forged by tests/gen/forged_proofs.py (every proof is valid under its own key).  One GPU, one process, warm.

    python tools/verify_mixed_ab.py > profiles/verify_mixed_ab.txt
"""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import plonkit_amd as pa  # noqa: E402
from oracle.oracle_lib import R_MOD  # noqa: E402
from tests.gen import forged_proofs as fp  # noqa: E402

DISTINCT = 16                                                        # proofs made per key; larger batches repeat them (every proof is verified on its own)
ROUNDS = 15
KEYS = 4


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def forge_keys(taus):
    """-> [(vk bytes, [proof bytes])], one key per tau, each with logarithms of its own"""
    out = []
    for k, tau in enumerate(taus):
        rng = random.Random("verify_mixed_ab key %d" % k)
        key = [rng.randrange(R_MOD) for _ in range(11)]
        made = [fp.forge_record(**dict(fp.random_args(rng, key=key), tau=tau)) for _ in range(DISTINCT)]
        assert all(f.valid and f.vk == made[0].vk for f in made)
        out.append((made[0].vk, [f.proof for f in made]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,16384")
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    a = ap.parse_args()
    ctx = pa.Context(0)
    L = pa.lib()
    print("# one plk_verify_mixed_packed call over %d keys vs %d plk_verify_many_packed calls, alternating, %d rounds each; ms, median (min .. max)" % (KEYS, KEYS, a.rounds))
    print("# events of the mixed call: front upload mul sum+affine pairing+settle download")
    print("# tables | proofs | mixed call | four calls, per round | sum of the four medians | events mixed")
    medians = {}
    for label, taus in (("one G2 pair", [42] * KEYS), ("four G2 pairs", [42, 5, 1, R_MOD - 1])):
        forged = forge_keys(taus)
        keys = [pa.VerificationKey(ctx, vk, strict_inputs=False) for vk, _ in forged]
        kset = pa.VerificationKeySet(ctx, keys)
        assert kset.keys == KEYS and kset.tables == len(set(taus))
        print("# %s: proofs of %d bytes, plk_vkset_tables = %d" % (label, len(forged[0][1][0]), kset.tables))
        for per_key in [int(x) for x in a.sizes.split(",")]:
            n = KEYS * per_key
            batch = [forged[i % KEYS][1][(i // KEYS) % DISTINCT] for i in range(n)]      # interleaved by key
            key_of = (np.arange(n, dtype=np.uint32) % KEYS).astype(np.uint32)
            blob = b"".join(batch)
            off = np.zeros(n + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(p) for p in batch], dtype=np.uint64)
            verdict = np.zeros(n, dtype=np.uint8)
            fb = ctypes.c_uint64(0)
            single = []                                               # per key: its proofs packed on their own, as a service that splits its inbox would hold them
            for k in range(KEYS):
                mine = batch[k::KEYS]
                o = np.zeros(per_key + 1, dtype=np.uint64)
                o[1:] = np.cumsum([len(p) for p in mine], dtype=np.uint64)
                single.append((b"".join(mine), o, np.zeros(per_key, dtype=np.uint8)))

            # through the C ABI with the arguments marshalled once: what is timed is the call
            def mixed():
                assert L.plk_verify_mixed_packed(ctx._h, kset._h, blob, ctypes.c_uint64(len(blob)), off.ctypes.data_as(ctypes.c_void_p), key_of.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.c_uint64(n), verdict.ctypes.data_as(ctypes.c_void_p), ctypes.byref(fb)) == 0

            def one(k):
                b, o, v = single[k]
                assert L.plk_verify_many_packed(ctx._h, keys[k]._h, b, ctypes.c_uint64(len(b)), o.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(per_key),
                                                v.ctypes.data_as(ctypes.c_void_p), ctypes.byref(fb)) == 0
            mixed()                                                   # warm: arena grown, code loaded, and every verdict "valid"
            assert verdict.all() and fb.value == 2 ** 64 - 1
            for k in range(KEYS):
                one(k)
                assert single[k][2].all()
            t_mixed, t_one = [], [[] for _ in range(KEYS)]
            for _ in range(a.rounds):
                t = time.perf_counter(); mixed(); t_mixed.append((time.perf_counter() - t) * 1e3)
                for k in range(KEYS):
                    t = time.perf_counter(); one(k); t_one[k].append((time.perf_counter() - t) * 1e3)
            ctx.set_kernel_timing(True)
            mixed()
            ev = ctx.verify_many_last_ms()
            ctx.set_kernel_timing(False)
            m = stats(t_mixed)
            rounds = stats([sum(t_one[k][r] for k in range(KEYS)) for r in range(a.rounds)])
            sum_med = sum(statistics.median(t_one[k]) for k in range(KEYS))
            medians[(label, per_key)] = (m, rounds, sum_med)
            print("%6d | %d x %5d | %9.2f (%.2f .. %.2f) | %9.2f (%.2f .. %.2f) | %9.2f | %s" % (
                kset.tables, KEYS, per_key, m[0], m[1], m[2], rounds[0], rounds[1], rounds[2], sum_med, " ".join("%.2f" % x for x in ev)))
        kset.close()
        for k in keys:
            k.close()
    if ("one G2 pair", 1024) in medians:
        m, rounds, sum_med = medians[("one G2 pair", 1024)]
        spread = rounds[2] - rounds[1]
        print("# condition at 4 x 1024 proofs of one G2 pair: mixed median %.2f < sum of the four medians %.2f - the sum's spread %.2f = %.2f : %s" % (
            m[0], sum_med, spread, sum_med - spread, "HOLDS" if m[0] < sum_med - spread else "DOES NOT HOLD"))
    for per_key in sorted(set(k[1] for k in medians)):
        if ("one G2 pair", per_key) in medians and ("four G2 pairs", per_key) in medians:
            a1, a4 = medians[("one G2 pair", per_key)][0][0], medians[("four G2 pairs", per_key)][0][0]
            print("# four tables against one at 4 x %d proofs: %.2f ms against %.2f ms (%+.1f %%)" % (per_key, a4, a1, 100.0 * (a4 - a1) / a1))
    print("done")


if __name__ == "__main__":
    main()
