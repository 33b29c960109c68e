#!/usr/bin/env python3
"""Per-kernel code-generation diff of two hipcc ``-S --cuda-device-only`` listings of
the same file (before / after a refactor): registers, LDS and scratch from the kernel
metadata, instruction count, and the opcodes whose counts differ. Prints one markdown
table row per kernel whose name contains one of the given substrings.

usage: python tools/asm_diff.py before.s after.s [kernel-substring ...]
"""
from __future__ import annotations

import collections
import re
import subprocess
import sys

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(path):
    """{symbol: (metadata dict, opcode Counter, [opcode, ...])}"""
    text = open(path).read().split("\n")
    meta, cur = {}, {}
    for ln in text:  # the amdhsa.kernels YAML at the end of the listing
        m = re.match(r"^\s+(?:- )?(\.\w+):\s+(\S+)$", ln)
        if m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".wavefront_size":  # the last key of a kernel's entry
                meta[cur[".name"]] = {k: int(cur[k]) for k in META}
                cur = {}
    out = {}
    starts = [(m.group(1), i) for i, ln in enumerate(text) if (m := re.match(r"^(_Z\S+):\s", ln))]
    for name, i in starts:
        if name not in meta:
            continue
        ops = []
        for ln in text[i + 1:]:
            m = re.match(r"^\t([a-z]\w+)", ln)
            if m:
                ops.append(m.group(1))
                if m.group(1) == "s_endpgm":
                    break
        out[name] = (meta[name], collections.Counter(ops), ops)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    want = sys.argv[3:] or [""]
    names = [n for n in a if any(w in n for w in want)]
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    print("| kernel | vgpr | sgpr | lds | scratch | instructions | opcodes that differ |")
    print("|---|---|---|---|---|---|---|")
    for n, d in zip(names, dem):
        d = re.sub(r"^void hipserve::|\(.*$", "", d)
        if n not in b:
            print(f"| `{d}` | missing after | | | | | |")
            continue
        (ma, ha, oa), (mb, hb, ob) = a[n], b[n]
        cols = [str(ma[k]) if ma[k] == mb[k] else f"{ma[k]} -> {mb[k]}" for k in META]
        cnt = str(len(oa)) if len(oa) == len(ob) else f"{len(oa)} -> {len(ob)}"
        diff = ", ".join(f"{op} {ha[op]} -> {hb[op]}" for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op])
        if not diff:
            diff = "none, same order" if oa == ob else "none (order differs)"
        print(f"| `{d}` | {' | '.join(cols)} | {cnt} | {diff} |")
    extra = [n for n in b if n not in a and any(w in n for w in want)]
    for n in extra:
        print(f"| `{n}` | new | | | | | |")


if __name__ == "__main__":
    main()
