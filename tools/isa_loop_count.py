#!/usr/bin/env python3
"""Counts the instructions of a kernel's hot loop from its gfx950 assembly (no GPU needed).

    python tools/isa_loop_count.py [--symbol SUBSTR] [--asm FILE.s | --src plonkit_amd/csrc/msm_accumulate.hip]

With --src the file is compiled to assembly with the flags of plonkit_amd/build.py (device side only).  The kernel whose
mangled name contains SUBSTR (default: msm_accumulate<6,2,false,false>) is cut into basic blocks; the ADDITION block is the block
with the most v_mad_u64_u32 among those with product-scanning wait states and no scratch access (or --block), the LOOP is the set of blocks on a cycle through it, and
the blocks executed EVERY iteration are those of the cycle through the addition block with the fewest VALU instructions (the
path of a wave none of whose lanes takes a cold branch).  Printed: per block the VALU instructions by mnemonic class, s_nop,
scratch accesses and code bytes; the per-iteration total; the register and occupancy lines of the kernel.
"""
import argparse
import collections
import heapq
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEFAULT_SYMBOL = "msm_accumulateILj6ELi2ELb0ELb0E"   # <6, 2, false, false>: the plain kernel without the infinity test (Lb0ELb1E: with it)


def compile_to_asm(src, out):
    sys.path.insert(0, ROOT)
    from plonkit_amd import build as b
    cmd = ["hipcc"] + b.FLAGS + b.FILE_FLAGS.get(os.path.basename(src), []) + ["-x", "hip", "--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)


def kernel_text(lines, sym):
    start = end = None
    for i, l in enumerate(lines):
        if start is None and re.match(r"^_Z\w*" + re.escape(sym) + r"\w*:", l):
            start = i
        elif start is not None and l.startswith(".Lfunc_end"):
            end = i
            break
    if start is None:
        raise SystemExit("no kernel matching %r" % sym)
    tail = []
    for l in lines[end:end + 80]:
        if re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy|codeLenInByte|LDSByteSize|TotalNumVgprs)", l):
            tail.append(l.strip())
    return lines[start + 1:end], tail


def blocks_of(body):
    """-> ordered dict label -> list of (mnemonic, operands); successors by label"""
    blocks, succ = collections.OrderedDict(), {}
    cur = "entry"
    blocks[cur] = []
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; (%bb\.\d+):", l)
        if m:
            nxt = m.group(1)
            succ.setdefault(cur, [])
            if not blocks[cur] or blocks[cur][-1][0] not in ("s_branch", "s_endpgm", "s_setpc_b64"):
                succ[cur].append(nxt)                          # fall through
            cur = nxt
            blocks[cur] = []
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        mn, ops = parts[0], parts[1] if len(parts) > 1 else ""
        blocks[cur].append((mn, ops))
        if mn.startswith("s_cbranch") or mn == "s_branch":
            succ.setdefault(cur, []).append(ops.strip())
    succ.setdefault(cur, [])
    return blocks, succ


def reach(succ, src, banned=()):
    seen, todo = set(), [s for s in succ.get(src, []) if s not in banned]
    while todo:
        x = todo.pop()
        if x in seen or x in banned:
            continue
        seen.add(x)
        todo.extend(succ.get(x, []))
    return seen


def inst_bytes(mn, ops):
    # enough for a size estimate: VOP3 / 64-bit encodings are 8 bytes, a literal adds 4; everything else 4
    if mn.startswith(("v_mad_u64", "v_lshrrev_b64", "v_lshlrev_b64", "v_mul_lo", "v_mul_hi", "v_alignbit", "v_or3", "v_and_or", "v_lshl_or", "v_lshl_add", "v_add3",
                      "v_bfe", "v_bfi", "v_cndmask_b32_e64", "v_cmp", "global_", "scratch_", "ds_", "flat_", "buffer_", "v_add_lshl", "v_xad", "v_sub_co", "v_add_co", "v_readlane", "v_writelane")) or mn.endswith("_e64"):
        n = 8
    else:
        n = 4
    if re.search(r"(^|[ ,])(0x[0-9a-f]{3,}|[0-9]{3,})($|,)", ops):
        n += 4
    return n


def classify(mn):
    for k in ("v_mad_u64_u32", "v_and_b32", "v_lshrrev_b64", "v_mul_lo_u32", "v_mov_b32", "v_alignbit_b32", "v_cndmask_b32", "v_or3_b32"):
        if mn.startswith(k):
            return k
    return "other VALU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbol", default=DEFAULT_SYMBOL)
    ap.add_argument("--asm")
    ap.add_argument("--src", default=os.path.join(ROOT, "plonkit_amd", "csrc", "msm_accumulate.hip"))
    ap.add_argument("--block", help="label of the addition block (default: see the source)")
    ap.add_argument("--all-blocks", action="store_true", help="also list the loop blocks that are NOT executed every iteration")
    a = ap.parse_args()
    if a.asm:
        lines = open(a.asm).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "k.s")
            compile_to_asm(a.src, out)
            lines = open(out).read().splitlines()
    body, tail = kernel_text(lines, a.symbol)
    blocks, succ = blocks_of(body)
    mads = lambda b: sum(1 for mn, _ in blocks[b] if mn.startswith("v_mad_u64_u32"))
    # The cold branches hold more multiply-adds than the mixed addition: the generic addition is built from the operand-scanning
    # products (no s_nop between their multiply-adds), and the doubling spills.  So: the block with the most multiply-adds among
    # those that have the wait states of the product-scanning chains and touch no scratch memory.
    nops = lambda b: sum(1 for mn, _ in blocks[b] if mn == "s_nop")
    cand = [b for b in blocks if nops(b) * 8 > mads(b) and not any(mn.startswith("scratch_") for mn, _ in blocks[b])]
    add = a.block or max(cand, key=mads)
    fwd = reach(succ, add)
    if add not in fwd:
        raise SystemExit("the addition block %s is not on a cycle" % add)
    loop = [b for b in blocks if b in fwd and add in reach(succ, b)]
    # the hot path: the cycle through the addition block with the fewest VALU instructions (what a wave executes when none
    # of its lanes takes a cold branch: the branches around cold code are s_cbranch_execz)
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
    path, b = [add], prev[add]
    while b != add:
        path.append(b)
        b = prev[b]
    every = [b for b in blocks if b in path]
    cols = ["v_mad_u64_u32", "v_and_b32", "v_lshrrev_b64", "v_mul_lo_u32", "v_mov_b32", "v_alignbit_b32", "v_cndmask_b32", "v_or3_b32", "other VALU"]
    print("kernel %s: %d blocks, loop through %s has %d blocks, %d executed every iteration" % (a.symbol, len(blocks), add, len(loop), len(every)))
    hdr = "%-12s %6s " % ("block", "VALU") + " ".join("%14s" % c for c in cols) + " %6s %8s %7s" % ("s_nop", "scratch", "bytes")
    print(hdr)
    tot = collections.Counter()

    def row(b, count):
        c = collections.Counter(classify(mn) for mn, _ in blocks[b] if mn.startswith("v_"))
        valu = sum(c.values())
        nop = sum(1 for mn, _ in blocks[b] if mn == "s_nop")
        scr = sum(1 for mn, _ in blocks[b] if mn.startswith("scratch_"))
        nbytes = sum(inst_bytes(mn, ops) for mn, ops in blocks[b])
        print("%-12s %6d " % (b + ("*" if b == add else ""), valu) + " ".join("%14d" % c[k] for k in cols) + " %6d %8d %7d" % (nop, scr, nbytes))
        if count:
            tot.update(c)
            tot["VALU"] += valu; tot["s_nop"] += nop; tot["scratch"] += scr; tot["bytes"] += nbytes

    for b in every:
        row(b, True)
    first = every.index(add)
    while first > 0 and every[first - 1].startswith("%bb") and every[first].startswith("%bb"):
        first -= 1
    last = every.index(add)
    while last + 1 < len(every) and every[last + 1].startswith("%bb"):
        last += 1
    grp = every[first:last + 1]
    print("addition (%s .. %s, contiguous): %d VALU, %d v_mad_u64_u32, %d s_nop, %d scratch" % (grp[0], grp[-1], sum(valu[b] for b in grp), sum(mads(b) for b in grp),
          sum(1 for b in grp for mn, _ in blocks[b] if mn == "s_nop"), sum(1 for b in grp for mn, _ in blocks[b] if mn.startswith("scratch_"))))
    print("%-12s %6d " % ("PER ITER", tot["VALU"]) + " ".join("%14d" % tot[k] for k in cols) + " %6d %8d %7d" % (tot["s_nop"], tot["scratch"], tot["bytes"]))
    if a.all_blocks:
        print("loop blocks off the every-iteration path (flush, special cases):")
        for b in loop:
            if b not in every:
                row(b, False)
    loop_bytes = sum(inst_bytes(mn, ops) for b in loop for mn, ops in blocks[b])
    print("loop code size (all %d blocks, estimate): %d bytes" % (len(loop), loop_bytes))
    for t in tail:
        print(t)


if __name__ == "__main__":
    main()
