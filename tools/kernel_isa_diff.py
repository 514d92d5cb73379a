#!/usr/bin/env python3
"""Which kernels of a .hip file a change moved, from two gfx950 assembly listings.

usage: python tools/kernel_isa_diff.py BEFORE.s AFTER.s
       (each made with: hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S FILE.hip -o X.s)

Splits each listing at its kernel symbols (.amdhsa_kernel names), strips comments and the
numbers of local labels (.LBB, .LJTI, .Ltmp, .Lfunc_*: they count up through the file, so
one changed kernel renumbers all behind it) and prints, per demangled kernel, `same`,
`DIFF a -> b lines`, `gone` or `new`, then the counts.  Text only: two builds of one source
give `same` for every kernel.
"""
import collections
import re
import subprocess
import sys

_LABEL = re.compile(r"\.L(BB|JTI|tmp|func_(?:begin|end))[0-9_]+")


def kernels(path):
    """{mangled kernel name: [normalised body lines]} of one listing."""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
        elif re.match(r"^\s*\.(section|text|rodata)\b", line):
            cur = None
        line = _LABEL.sub(r".L\1", re.sub(r"\s*(;|//).*", "", line)).strip()
        if cur is not None and line:
            cur.append(line)
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    order = list(a) + [k for k in b if k not in a]
    pretty = subprocess.run(["c++filt"], input="\n".join(order), capture_output=True, text=True).stdout.split("\n")
    count = collections.Counter()
    for k, name in zip(order, pretty):
        what = ("new" if k not in a else "gone" if k not in b else "same" if a[k] == b[k]
                else f"DIFF {len(a[k])} -> {len(b[k])} lines")
        count[what.split()[0]] += 1
        print(f"{what:28s} {re.sub(r'[(].*', '', name)}")
    print(", ".join(f"{n} {w}" for w, n in sorted(count.items())))
