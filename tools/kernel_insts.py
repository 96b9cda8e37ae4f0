#!/usr/bin/env python
"""Instruction mix per basic block of one kernel in a gfx950 assembly listing: where a kernel's issue slots go, without a GPU.
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Idifacto_amd/csrc --cuda-device-only -S -o api.s difacto_amd/csrc/dfh_api.hip
  python tools/kernel_insts.py api.s _ZN3dfh10k_loc_sortENS_7LocViewE [min instructions per block]
VALU = v_* (v_readlane / DPP / v_permlane*_swap moves included), LDS = ds_*, VMEM = global_ / flat_ / buffer_, SMEM = s_load*,
wait = s_waitcnt / s_nop / s_barrier, SALU = every other s_*.  A block's loop depth is the compiler's own comment."""
import re
import sys


def blocks(path, fn):
    t = open(path).read()
    a = t.index(fn + ":")
    out = [["entry", "", []]]
    for raw in t[a:t.index(".Lfunc_end", a)].split("\n")[1:]:
        m = re.match(r"(\.LBB\d+_\d+):|; %bb\.(\d+):", raw)
        if m:
            d = re.search(r"Depth=(\d+)", raw)
            out.append([m.group(1) or "%bb." + m.group(2), "depth " + d.group(1) if d else "", []])
            continue
        d = re.search(r"Inner Loop Header: Depth=(\d+)", raw)
        if d:
            out[-1][1] = "inner loop, depth " + d.group(1)
        l = raw.split(";")[0].strip()
        if l and not l.startswith("."):
            out[-1][2].append(l)
    return out


def cls(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op in ("s_waitcnt", "s_nop", "s_barrier"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
        return "branch"
    if op.startswith("s_load"):
        return "SMEM"
    return "SALU" if op.startswith("s_") else "other"


def main(path, fn, least=0):
    cols = ("VALU", "SALU", "LDS", "VMEM", "SMEM", "wait", "branch")
    marks = ("v_readlane", "_dpp", "v_permlane", "ds_read", "ds_write", "global_load", "global_store", "s_barrier")
    print("%-12s %-20s " % ("block", "loop") + " ".join("%6s" % c for c in cols) + "  of which")
    tot = dict.fromkeys(cols, 0)
    for name, depth, ins in blocks(path, fn):
        c = dict.fromkeys(cols + ("other",), 0)
        for i in ins:
            c[cls(i.split()[0])] += 1
        for k in cols:
            tot[k] += c[k]
        if len(ins) < int(least):
            continue
        m = ", ".join("%d %s" % (n, k) for k in marks for n in [sum(k in i for i in ins)] if n)
        print("%-12s %-20s " % (name, depth) + " ".join("%6d" % c[k] for k in cols) + "  " + m)
    print("%-12s %-20s " % ("kernel", "") + " ".join("%6d" % tot[k] for k in cols))


if __name__ == "__main__":
    main(*sys.argv[1:])
