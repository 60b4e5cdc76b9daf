#!/usr/bin/env python3
"""Compares two builds' gfx950 assembly kernel by kernel (no GPU):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S pyz_api.hip -o build.s      (in each tree's csrc/)
    python tools/asm_compare.py parent.s branch.s

A kernel is "identical" when its text between its label and its end marker -- instructions, the kernel descriptor, the
compiler's comments -- is the same line for line once the function numbers inside basic-block labels (.LBB12_3, BB12_3) and
temporary labels, and the run lengths of blanks (the alignment of comments shifts with the digits of those numbers), are
normalised.  Prints one JSON object: the counts, the kernels that differ, those missing and those new."""

import json
import re
import sys


def functions(path):
    out, isfunc, name, buf = {}, set(), None, []
    for line in open(path):
        t = re.match(r"^\s*\.type\s+(\S+),@function", line)
        if t:
            isfunc.add(t.group(1))
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if name is None:
            if m and m.group(1) in isfunc:
                name, buf = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = buf, None
        else:
            buf.append(re.sub(r"[ \t]+", " ", re.sub(r"BB\d+_", "BB_", re.sub(r"\.Ltmp\d+", ".Ltmp", line))))
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])

    def kernel(buf):
        return any(".amdhsa_kernel" in line for line in buf)
    kern = sorted(k for k in a if kernel(a[k]))
    print(json.dumps({"parent_kernels": len(kern),
                      "identical_line_for_line": sum(1 for k in kern if k in b and a[k] == b[k]),
                      "differ": [k for k in kern if k in b and a[k] != b[k]],
                      "missing_in_branch": [k for k in kern if k not in b],
                      "new_in_branch": sorted(k for k in b if k not in a and kernel(b[k]))}, indent=1))


if __name__ == "__main__":
    main()
