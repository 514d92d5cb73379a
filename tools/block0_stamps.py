#!/usr/bin/env python3
"""Where block 0 of a k_gemm level stands against the level's other workgroups, from a
diagnostic timeline dump (SACMI_DIAG_DUMP of a -DSACMI_DIAG_PHASES build, as tools/phase_dump.py
reads it).  Per site whose name contains one of the given substrings, the median over the
dumped updates of (us from the kernel's first entry):
  last      the workgroup that leaves last, per update
  end med / max / b0   workgroup exits (phase 5): median, latest, block 0's
  b0 w0     block 0, wave 0: entry, K-loop start (behind the scalar chain of a fused-Adam
            level), K-loop end
  b0 wL     block 0's last wave: entry, K-loop end
  med w0    the same three clocks of wave 0, median over all workgroups
Only tile workgroups count; where a ride workgroup ran the level's scalar chain, a second line
gives its entry (the chain's start) and the chain's end.
usage: tools/block0_stamps.py dump.bin L6 L13"""
import struct
import sys

import numpy as np


def main(path, pats):
    raw = open(path, "rb").read()
    sites, per, words, nph = struct.unpack("4q", raw[:32])
    names = [raw[32 + 32 * i:64 + 32 * i].split(b"\0")[0].decode() for i in range(sites)]
    w = np.frombuffer(raw[32 + 32 * sites:], np.uint64).reshape(sites, per, words)
    acc, chains = {}, {}
    for s in range(sites):
        x = w[s, 0]
        if not any(p in names[s] for p in pats) or x[0] == 2**64 - 1 or int(x[2]) != 1 or nph < 8:
            continue
        p0 = words - 256 * nph
        ph = x[p0:p0 + 256 * nph].reshape(256, nph).astype(np.int64)
        live = np.nonzero((ph[:, 0] > 0) & (ph[:, 5] > 0))[0]      # the tile workgroups
        # (an unstamped word keeps the buffer's all-ones: -1 here)
        ride = np.nonzero((ph[:, 0] > 0) & (ph[:, 5] <= 0) & (ph[:, 2] > 0))[0]
        if len(ride):     # a ride workgroup that ran the level's scalar chain: entry, chain end
            r = (ph[ride[0]] - int(x[0])) * 0.01
            chains.setdefault(names[s], []).append((int(ride[0]), r[0], r[2]))
        ph = (ph[live] - int(x[0])) * 0.01
        b0 = int(np.nonzero(live == 0)[0][0])
        row = [int(x[3]), len(live), np.median(ph[:, 5]), np.max(ph[:, 5]), ph[b0, 5],
               ph[b0, 0], ph[b0, 1], ph[b0, 2], ph[b0, 6], ph[b0, 7],
               np.median(ph[:, 0]), np.median(ph[:, 1]), np.median(ph[:, 2])]
        acc.setdefault(names[s], []).append((int(live[np.argmax(ph[:, 5])]), row))
    print(f"{'site':28s} {'grid':>4s} {'wgs':>4s} {'last':>14s} {'end med':>7s} {'max':>6s} {'b0':>6s} | "
          f"{'b0 w0 in':>8s} {'K0':>6s} {'K1':>6s} | {'b0 wL in':>8s} {'K1':>6s} | {'med w0 in':>9s} "
          f"{'K0':>6s} {'K1':>6s}")
    for n, lst in acc.items():
        m = np.median(np.array([r for _, r in lst]), axis=0)
        last = ",".join(str(b) for b, _ in lst)
        print(f"{n:28s} {int(m[0]):4d} {int(m[1]):4d} {last:>14s} {m[2]:7.2f} {m[3]:6.2f} {m[4]:6.2f} | "
              f"{m[5]:8.2f} {m[6]:6.2f} {m[7]:6.2f} | {m[8]:8.2f} {m[9]:6.2f} | {m[10]:9.2f} "
              f"{m[11]:6.2f} {m[12]:6.2f}")
    for n, lst in chains.items():
        m = np.median(np.array([r[1:] for r in lst]), axis=0)
        print(f"{n:28s} chain on ride workgroup {lst[0][0]}: entry {m[0]:.2f} chain end {m[1]:.2f}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:] or ["L6", "L13"])
