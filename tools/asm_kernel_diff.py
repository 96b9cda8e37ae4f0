#!/usr/bin/env python3
"""Compare two device listings of the library kernel by kernel (a host-side refactor must leave every kernel as it was).
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-value -Iinclude -Idifacto_amd/csrc --cuda-device-only -S -o api.s difacto_amd/csrc/dfh_api.hip
  python tools/asm_kernel_diff.py parent/api.s api.s
Host code that moves changes the order in which templates are instantiated, hence the order of the functions in the listing and
the ordinals in their local labels; nothing else may differ.  Equal: the set of function names, every function's body and every
kernel's descriptor, after the ordinals are replaced."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        if line.startswith(("\t.file", "\t.ident")) or "__hip_cuid_" in line:
            continue
        m = re.match(r"\t\.(?:type\t(\S+),@function|amdhsa_kernel (\S+))", line)
        if m:
            name, body = (m.group(1) or "desc:" + m.group(2)), []
            out[name] = body
        if name:
            line = re.sub(r"((?:\.L)?BB|\.L(?:func_end|func_begin|tmp|JTI)|\$__internal_)\d+", r"\1#", line)
            body.append(re.sub(r"\s+;", " ;", line))   # (the column of a label's comment moves with the ordinal's width)
            if line.startswith(("\t.end_amdhsa_kernel", ".Lfunc_end")):
                name = None
    return out


a, b = functions(sys.argv[1]), functions(sys.argv[2])
bad = sorted(set(a) ^ set(b)) + sorted(n for n in set(a) & set(b) if a[n] != b[n])
print("%d functions and descriptors in %s, %d in %s, %d differ" % (len(a), sys.argv[1], len(b), sys.argv[2], len(bad)))
for n in bad[:20]:
    print("  ", n)
sys.exit(1 if bad else 0)
