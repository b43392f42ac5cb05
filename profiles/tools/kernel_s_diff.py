#!/usr/bin/env python3
"""Compare two device assembly listings of bhray_kernels.hip (hipcc --cuda-device-only -S) KERNEL BY KERNEL.

A flat `diff` of two listings is useless when the instantiation order changed (the function numbers in the labels
and the order of the sections move): this splits each listing into its functions, drops what only numbers them
(.LBB<n>_ / .Lfunc_end<n> / .Lfunc_begin<n>), optionally rewrites the kernel names with a regular expression
(--strip: e.g. a template parameter one tree has and the other has not) and reports, per function name, whether the
instruction text is the same.  Hand-run (profiles/EXPERIMENTS.md R10.1); not a test.

  kernel_s_diff.py parent.s stand_in.s --strip 'ELb0E(?=EvPKNS_11FrameParams)' --to 'E'
"""
import argparse
import re
import sys


def functions(path, strip, to):
    text = open(path).read()
    if strip:
        text = re.sub(strip, to, text)
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))
        body = re.sub(r"\.Lfunc_(begin|end)\d+", ".Lfunc", body)
        lines = [re.sub(r"\s*;.*$", "", ln) for ln in body.split("\n")]      # comments number the functions too ("in Loop: Header=BB37_5")
        out[m.group(1)] = [ln for ln in lines if ln.strip()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a"); ap.add_argument("b")
    ap.add_argument("--strip", default=""); ap.add_argument("--to", default="")
    ap.add_argument("--only", default="", help="regular expression: the function names to compare")
    a = ap.parse_args()
    fa, fb = functions(a.a, a.strip, a.to), functions(a.b, a.strip, a.to)
    names = sorted(n for n in set(fa) | set(fb) if re.search(a.only, n))
    same = differ = 0
    for n in names:
        if n not in fa or n not in fb:
            print(f"ONLY IN {'A' if n in fa else 'B'}  {n}  ({len(fa.get(n) or fb.get(n))} lines)")
            continue
        if fa[n] == fb[n]:
            same += 1
            print(f"same      {len(fa[n]):6d} lines  {n}")
        else:
            differ += 1
            nd = sum(1 for x, y in zip(fa[n], fb[n]) if x != y) + abs(len(fa[n]) - len(fb[n]))
            print(f"DIFFERENT {len(fa[n]):6d} / {len(fb[n]):6d} lines, {nd} differ  {n}")
    print(f"{same} functions identical, {differ} different, of {len(names)}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
