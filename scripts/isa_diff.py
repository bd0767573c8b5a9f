"""Compare two gfx950 assembly files (hipcc --cuda-device-only -S) kernel by kernel.

Usage:  python scripts/isa_diff.py before.s after.s

Per kernel symbol: the instruction text between the symbol's label and its
.Lfunc_end label, and its .amdhsa_kernel descriptor block (VGPRs, SGPRs, LDS,
scratch, ...).  Symbol order, .file / .ident lines and the per-function
ordinal in local labels (.LBB<n>_, .Lfunc_end<n>) do not count.  Exit status 0
when both files hold the same kernels with identical text and descriptors.
"""
from __future__ import annotations

import re
import sys

_ORD = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|LCPI)\d+")


def kernels(path: str) -> dict:
    out, desc = {}, {}
    sym, body, dsym, dlines = None, [], None, []
    for line in open(path):
        line = _ORD.sub(r".\1", line.rstrip())
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            dsym, dlines = m.group(1), []
        elif dsym is not None:
            if line.strip() == ".end_amdhsa_kernel":
                desc[dsym], dsym = dlines, None
            else:
                dlines.append(line.strip())
        elif sym is None:
            m = re.match(r"(\w+):\s*; @\1$", line)
            if m:
                sym, body = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            out[sym], sym = body, None
        else:
            body.append(line)
    return {k: (out[k], desc[k]) for k in desc}  # kernels only (device functions have no descriptor)


def main() -> int:
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print(("lost   " if k in a else "gained ") + k)
    for k in sorted(set(a) & set(b)):
        if a[k][0] != b[k][0]:
            print("text differs        " + k)
            bad.append(k)
        elif a[k][1] != b[k][1]:
            print("descriptor differs  " + k)
            bad.append(k)
    print(f"kernels: {len(a)} before, {len(b)} after; {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
