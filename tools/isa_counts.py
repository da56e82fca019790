#!/usr/bin/env python3
"""Static instruction counts per kernel of a device assembly listing (hipcc --cuda-device-only -S):
  tools/isa_counts.py <file.s> [symbol filter ...]
VALU = v_* (without the lane exchanges counted on their own), SALU = s_* without waits / nops / branches / barriers.
A static count is a dynamic one only for straight-line code every wave runs once (profiles/frontier_uniform_isa.txt)."""
import re
import sys

NOT_ALU = ("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_barrier", "s_endpgm", "s_sleep", "s_setprio", "s_load", "s_buffer_load",
           "s_memtime", "s_code_end")


def main():
    path, filters = sys.argv[1], sys.argv[2:]
    name, rows, cur = None, [], None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            cur = dict(valu=0, salu=0, div_fixup=0, readlane=0, writelane=0)
            rows.append((name, cur))
            continue
        if cur is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        op = line.strip().split(" ")[0].split("\t")[0]
        if op.startswith("v_"):
            cur["valu"] += 1
            if op.startswith("v_div_fixup"):
                cur["div_fixup"] += 1
            elif op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
                cur["readlane"] += 1
            elif op.startswith("v_writelane"):
                cur["writelane"] += 1
        elif op.startswith("s_") and not op.startswith(NOT_ALU):
            cur["salu"] += 1
    for name, c in rows:
        if filters and not any(f in name for f in filters):
            continue
        print("%-80s VALU %5d SALU %5d v_div_fixup %3d v_readlane %4d v_writelane %4d" %
              (name[-80:], c["valu"], c["salu"], c["div_fixup"], c["readlane"], c["writelane"]))


if __name__ == "__main__":
    main()
