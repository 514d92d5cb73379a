#!/usr/bin/env python3
"""Per-kernel register / spill / scratch / occupancy table from hipcc's resource remarks.

usage: python tools/kernel_resources.py csrc/kernels.hip [more .hip] [--match SUBSTR]
       (run from the package dir)

Columns: VGPRs, AGPRs, SGPRs, SGPR spills (the compiler parks them in VGPR lanes: each
costs a v_writelane where it is saved and a v_readlane wherever it is used again), VGPR
spills, scratch bytes per lane, occupancy, LDS bytes.  --match keeps the kernels whose
demangled name contains SUBSTR.
"""
import re
import subprocess
import sys

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-c", "-o", "/dev/null",
         "-Rpass-analysis=kernel-resource-usage"]
# remark label -> row key
FIELDS = {"VGPRs": "VGPRs", "AGPRs": "AGPRs", "TotalSGPRs": "SGPRs", "SGPRs": "SGPRs", "SGPRs Spill": "SGPRSpill",
          "VGPRs Spill": "VGPRSpill", "ScratchSize [bytes/lane]": "ScratchSize",
          "Occupancy [waves/SIMD]": "Occupancy", "LDS Size [bytes/block]": "LDS"}
_FIELD_RE = re.compile(r"remark:\s+(" + "|".join(re.escape(k) for k in sorted(FIELDS, key=len, reverse=True))
                       + r"): (\d+)")


def parse(remarks):
    """Rows (one dict per kernel) from the text of hipcc's kernel-resource-usage remarks."""
    rows, cur = [], None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        m = _FIELD_RE.search(line)
        if m and cur is not None:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return rows


def table(src):
    return parse(subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, src], capture_output=True, text=True).stderr)


def demangle(name):
    out = subprocess.run(["c++filt"], input=name, capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*", "", out)


def fmt(r, name):
    return (f"{r.get('VGPRs', 0):4d} v {r.get('AGPRs', 0):3d} a {r.get('SGPRs', 0):3d} s "
            f"{r.get('SGPRSpill', 0):3d} sspill {r.get('VGPRSpill', 0):3d} vspill "
            f"{r.get('ScratchSize', 0):4d} scr occ {r.get('Occupancy', 0)} lds {r.get('LDS', 0):6d}  {name}")


if __name__ == "__main__":
    args = sys.argv[1:]
    match = None
    if "--match" in args:
        i = args.index("--match")
        match = args[i + 1]
        del args[i:i + 2]
    for src in args:
        for r in table(src):
            name = demangle(r["name"])
            if match is None or match in name:
                print(fmt(r, name))
