#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two builds' device code (profiles/cx_host_refactor.txt).

    hipcc <product flags> --cuda-device-only -S file.hip -o DIR/file.s      # once per source tree
    python scratch/isa_compare.py DIR_A DIR_B cx_report mhl_report ...

Kernels are matched by demangled name without argument types (k_cx_tiles: without a trailing `, 0` template argument);
mangled names and basic-block label numbers are replaced by placeholders.  A kernel counts as identical when instruction
stream, kernel descriptor and the resource lines of the metadata are equal; for the others the resource lines are printed,
and the differing lines are classed as "kernel-argument offset" (the same s_load / s_add / kernarg_size line with another
immediate) or "other".
"""
import os
import re
import subprocess
import sys

RES = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def parse(path):
    txt = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    md = txt[txt.index(".amdgpu_metadata"):]
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count", md)[1:]:
        meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = {k: int(re.search(r"%s:\s+(\d+)" % re.escape(k), blk).group(1)) for k in RES}
    for n, d in zip(names, dem):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\t\.section\t\.rodata" % re.escape(n), txt, re.M | re.S).group(1)
        desc = re.search(r"\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(n), txt, re.S).group(1)
        text = body + desc
        for m in sorted(names, key=len, reverse=True):
            text = text.replace(m, "KERNEL")
        text = re.sub(r"BB\d+_", "BB_", text)                      # labels, and the loop headers named in comments
        text = re.sub(r"[ \t]+;", " ;", text)                      # (comments are aligned to the label's width)
        key = re.sub(r"(k_cx_tiles<.*), 0>$", r"\1>", d.split("(")[0])
        out[key] = (text.split("\n"), meta[n])
    return out


def main():
    total = same = 0
    for f in sys.argv[3:]:
        a, b = parse(os.path.join(sys.argv[1], f + ".s")), parse(os.path.join(sys.argv[2], f + ".s"))
        if set(a) != set(b):
            print(f, "kernel sets differ:", sorted(set(a) ^ set(b)))
        differ = []
        for k in sorted(set(a) & set(b)):
            (ta, ma), (tb, mb) = a[k], b[k]
            total += 1
            if ta == tb and ma == mb:
                same += 1
                continue
            arg = other = 0
            if len(ta) != len(tb):
                other = abs(len(ta) - len(tb))
            for x, y in zip(ta, tb):
                if x != y:
                    cut = lambda t: re.sub(r"(0x[0-9a-f]+|\d+)$", "", t)
                    if cut(x) == cut(y) and re.match(r"\s*(s_load_dword|s_add_u32|\.amdhsa_kernarg_size)", x): arg += 1
                    else: other += 1
            differ.append((k, ma, mb, arg, other))
        print("%-12s %3d kernels, %3d identical, %3d differ" % (f, len(a), len(a) - len(differ), len(differ)))
        for k, ma, mb, arg, other in differ:
            print("  %s: %d kernel-argument offset lines, %d other lines; resources %s" %
                  (k, arg, other, "equal " + str(list(ma.values())) if ma == mb else "DIFFER %s -> %s" % (ma, mb)))
    print("total: %d kernels, %d identical" % (total, same))


if __name__ == "__main__":
    main()
