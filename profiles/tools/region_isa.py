#!/usr/bin/env python3
"""Vector instructions of a trace kernel PER REGION of the round - refill, march (plain step / rare path), general step, disk shading, flat passes, epilogue -
from a `hipcc --cuda-device-only -S -gline-tables-only` listing of bhray_kernels.hip (line tables do not change the instructions: the totals equal the listing
without them).  Every instruction is attributed through the OUTERMOST frame of its .loc's inlined-at chain (`; file:line:col @[ ... @[ bhray_kernels.hip:line:col ] ]`):
the line of trace_kernel - or of the step's .inc file - that the instruction was inlined into, so `shade_disk`, `bh_atan2` or a bilinear sample count for the phase
that called them.  The regions' line ranges are read from the source's own phase comments (`// ---- refill ...`).  An instruction whose location is line 0 (the
compiler's own) counts for the region of the instruction before it.  Hand-run (profiles/EXPERIMENTS.md R15.1); not a test.

  region_isa.py kernels_g.s bhusie_amd/csrc/bhray_kernels.hip 'trace_kernel<1, false, false, true, 0, true, false>'
"""
import collections
import re
import subprocess
import sys


def regions_of(src_path):
    src = open(src_path).read().split("\n")

    def line(marker, after=0):
        for i, l in enumerate(src):
            if i >= after and marker in l:
                return i + 1
        raise SystemExit(f"marker not found: {marker}")
    k = line("void trace_kernel(const FrameParams*")
    refill = line("// ---- refill finished lanes", k)
    refill_end = line("if (!__any(mode != M_EMPTY))", refill)
    lens = line("// ---- lensed meshes", refill_end)
    shade = line("// ---- deferred disk shading", lens)
    flat = line("// ---- flat-space iterations", shade)
    epi = line("// ---- epilogue", flat)
    epi_end = line("mode = M_EMPTY;", epi)
    return [("refill", refill, refill_end), ("lens phase", lens, shade - 1), ("disk shading", shade, flat - 1), ("flat passes", flat, epi - 1), ("epilogue", epi, epi_end)]


def rare_path_line(inc_path):
    for i, l in enumerate(open(inc_path).read().split("\n")):
        if "if (near_horizon || near_disk || cd > H.R" in l:
            return i + 1
    raise SystemExit("rare-path test not found in " + inc_path)


def main():
    path, src_path, want = sys.argv[1], sys.argv[2], sys.argv[3]
    regs = regions_of(src_path)
    csrc = src_path.rsplit("/", 1)[0]
    rare_u = rare_path_line(csrc + "/bhray_step_u.inc")
    text = open(path).read()
    body = None
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        if want in subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout:
            body = m.group(2)
            break
    assert body, "kernel not found"
    count, divs = collections.Counter(), collections.Counter()
    region, depth = "prologue / frame loop / end", 0
    for l in body.split("\n"):
        b = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", l) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", l)
        if b:
            d = re.search(r"Depth=(\d+)", b.group(2) or "")
            depth = int(d.group(1)) if d else 0
            continue
        m = re.match(r"^\t\.loc\t\d+ (\d+) \d+.*?; (.*)$", l)
        if m:
            frames = re.findall(r"([\w./+-]+):(\d+):\d+", m.group(2))
            if not frames:
                continue
            f, n = frames[-1][0].rsplit("/", 1)[-1], int(frames[-1][1])
            if n == 0:
                continue
            if f == "bhray_step_u.inc":
                region = "march: unified step, plain" if n < rare_u else "march: unified step, rare path"
            elif f == "bhray_step.inc":
                region = "general step (odd lanes; behind the flat pass)"
            elif f == "bhray_march.inc":
                region = "march: loop, odd test, state fix-up"
            elif f == "bhray_kernels.hip":
                region = "prologue / frame loop / end"
                for name, a, z in regs:
                    if a <= n <= z:
                        region = name
            continue
        if l.startswith("\t") and not l.strip().startswith((";", ".")):
            op = l.strip().split()[0]
            if op.startswith("v_"):
                count[region] += 1
            if op.startswith("v_div_fixup"):
                divs[region] += 1
    print(want)
    for r in sorted(count, key=lambda r: -count[r]):
        print(f"  {r:48s} vector instructions {count[r]:5d}   IEEE divisions {divs[r]:3d}")
    print(f"  {'total':48s} vector instructions {sum(count.values()):5d}   IEEE divisions {sum(divs.values()):3d}")


main()
