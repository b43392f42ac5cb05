#!/usr/bin/env python3
"""Summarise a rocprofv3 --pmc run of bench.py per trace launch of the ladder: medians of every counter over the dispatches of
levels 0+1, level 2 and level 3 (a dispatch is told by its SQ_INSTS_VALU: the three launches of a 1080p frame are a factor
of two and of six apart), and SQ_INSTS_VALU per frame.  Hand-run (profiles/EXPERIMENTS.md R11.1); not a test.

  pmc_levels.py LABEL DIR     (DIR: the -d directory of the run; reads every *counter_collection.csv below it)
"""
import collections
import csv
import glob
import statistics
import sys


def main():
    label, d = sys.argv[1], sys.argv[2]
    disp = collections.defaultdict(dict); kern = {}
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "trace_kernel" not in r["Kernel_Name"]:
                continue
            k = (f, r["Dispatch_Id"])
            disp[k][r["Counter_Name"]] = disp[k].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            kern[k] = r["Kernel_Name"].split("(")[0]
    print(f"== {label}: {len(disp)} trace dispatches, kernels {dict(collections.Counter(kern.values()))}")
    lv = collections.defaultdict(lambda: collections.defaultdict(list))
    for k, c in disp.items():
        v = c.get("SQ_INSTS_VALU", 0.0)
        name = "levels 0+1" if v < 30e6 else "level 2   " if v < 100e6 else "level 3   "
        for n, x in c.items():
            lv[name][n].append(x)
    frame = 0.0
    for name in sorted(lv):
        for n in ("SQ_INSTS_VALU", "SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES"):
            xs = lv[name].get(n, [])
            if xs:
                print(f"   {name} {n:15s} n={len(xs):3d} median {statistics.median(xs):14.0f}  min {min(xs):14.0f}  max {max(xs):14.0f}")
        frame += statistics.median(lv[name]["SQ_INSTS_VALU"])
    print(f"   SQ_INSTS_VALU per frame (all three trace launches): {frame:.0f}")


if __name__ == "__main__":
    main()
