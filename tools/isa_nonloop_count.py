#!/usr/bin/env python3
"""Counts, from the gfx950 assembly of msm.hip (no GPU needed), the VALU instructions of the kernels around msm_accumulate:

    python tools/isa_nonloop_count.py [--asm FILE.s | --src plonkit_amd/csrc/msm.hip] [--reduce SUBSTR ...]

  * msm_task_reduce (every instantiation whose mangled name contains one of --reduce; default <6,4,...> and <6,5,...>): the ONE
    full addition of the step loop = the blocks on the cycle with the fewest VALU instructions through the block that holds the
    most v_mad_u64_u32 (the path of a wave none of whose lanes takes a cold branch), multiply-adds and the rest apart, with the
    scratch accesses on that path, and the register / occupancy lines of the kernel;
  * msm_recode_count and msm_recode_scatter: the straight-line code = every block that is on no cycle (the copy-out loops and
    the scan loops are left out), per scalar (the count kernel takes RC_COUNT_PER = 4 scalars per thread, the scatter kernel
    one).  The count is static: both arms of a branch are counted (the "whole wave holds one scalar" arm of the two kernels is
    ~15 x 6 instructions per scalar that a wave of distinct scalars does not execute).
Compiled with the flags of plonkit_amd/build.py, as tools/isa_loop_count.py does.
"""
import argparse
import heapq
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import isa_loop_count as ilc  # noqa: E402

ROOT = ilc.ROOT
RECODE = (("msm_recode_count", 4), ("msm_recode_scatter", 1))


def split(insts):
    valu = [mn for mn, _ in insts if mn.startswith("v_")]
    mads = sum(1 for mn in valu if mn.startswith("v_mad_u64_u32"))
    return len(valu), mads, len(valu) - mads


def hot_cycle(blocks, succ, add):
    valu = {b: sum(1 for mn, _ in blocks[b] if mn.startswith("v_")) for b in blocks}
    dist, prev, heap = {}, {}, [(0, i, s, add) for i, s in enumerate(succ[add])]
    heapq.heapify(heap)
    while heap:
        d, _, b, frm = heapq.heappop(heap)
        if b in dist:
            continue
        dist[b], prev[b] = d, frm
        if b == add:
            break
        for i, s2 in enumerate(succ.get(b, [])):
            if s2 not in dist:
                heapq.heappush(heap, (d + valu[b], i, s2, b))
    if add not in prev:
        raise SystemExit("the addition block %s is not on a cycle" % add)
    path, b = [add], prev[add]
    while b != add:
        path.append(b)
        b = prev[b]
    return [b for b in blocks if b in path]


def reduce_report(lines, sym):
    body, tail = ilc.kernel_text(lines, sym)
    blocks, succ = ilc.blocks_of(body)
    mads = lambda b: sum(1 for mn, _ in blocks[b] if mn.startswith("v_mad_u64_u32"))
    add = max(blocks, key=mads)
    path = hot_cycle(blocks, succ, add)
    # the addition = the blocks of the path that hold multiply-adds (the operand selection in front of it is the step loop's)
    first = min(i for i, b in enumerate(path) if mads(b))
    last = max(i for i, b in enumerate(path) if mads(b))
    grp = path[first:last + 1]
    insts = [x for b in grp for x in blocks[b]]
    v, m, r = split(insts)
    nop = sum(1 for mn, _ in insts if mn == "s_nop")
    scr = sum(1 for mn, _ in insts if mn.startswith("scratch_"))
    vs, ms, rs = split([x for b in path for x in blocks[b]])
    print("%s: addition blocks %s .. %s (%d blocks): %d VALU = %d v_mad_u64_u32 + %d other; %d s_nop, %d scratch" % (sym, grp[0], grp[-1], len(grp), v, m, r, nop, scr))
    print("%s: whole step (%d blocks executed every step): %d VALU = %d v_mad_u64_u32 + %d other" % (sym, len(path), vs, ms, rs))
    # one addition site: the kernel holds the multiply-adds of ONE addition, one doubling (its cold branch, ~1270) and the exact zero tests (162 each)
    print("%s: v_mad_u64_u32 in the whole kernel: %d" % (sym, sum(mads(b) for b in blocks)))
    for t in tail:
        print("    " + t)
    return v


def recode_report(lines, sym, per_thread):
    body, tail = ilc.kernel_text(lines, sym)
    blocks, succ = ilc.blocks_of(body)
    straight = [b for b in blocks if b not in ilc.reach(succ, b)]
    v, m, r = split([x for b in straight for x in blocks[b]])
    print("%s: straight-line code (%d of %d blocks), %d scalar(s) per thread: %d VALU = %d v_mad_u64_u32 + %d other  ->  per scalar %.1f = %.1f + %.1f"
          % (sym, len(straight), len(blocks), per_thread, v, m, r, v / per_thread, m / per_thread, r / per_thread))
    for t in tail:
        print("    " + t)
    return v / per_thread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--src", default=os.path.join(ROOT, "plonkit_amd", "csrc", "msm.hip"))
    ap.add_argument("--reduce", nargs="*", default=["msm_task_reduceILj6ELj4E", "msm_task_reduceILj6ELj5E"])
    a = ap.parse_args()
    if a.asm:
        lines = open(a.asm).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "k.s")
            ilc.compile_to_asm(a.src, out)
            lines = open(out).read().splitlines()
    syms = sorted({l.split(":")[0] for l in lines if l.startswith("_Z") and any(s in l.split(":")[0] for s in a.reduce)})
    for s in syms:
        reduce_report(lines, s[2:])
    total = 0.0
    for s, per in RECODE:
        total += recode_report(lines, s, per)
    print("recode kernels together, per scalar: %.1f VALU" % total)


if __name__ == "__main__":
    main()
