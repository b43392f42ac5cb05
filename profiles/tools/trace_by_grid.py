"""Per-launch kernel durations of a `rocprofv3 --kernel-trace --output-format csv` run, grouped by kernel and grid size: the ladder's trace launches share one kernel
name, and with the trace grids sized by queue length (EXPERIMENTS R13.1) the grid tells the levels apart.  usage: python profiles/tools/trace_by_grid.py <kernel_trace.csv> [first_dispatches_to_skip]"""
import csv
import re
import statistics as st
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 0
grid_col = next(c for c in rows[0] if c in ("Grid_Size_X", "Grid_Size"))
wg_col = next((c for c in rows[0] if c in ("Workgroup_Size_X", "Workgroup_Size")), None)
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
groups = {}
for r in rows[skip:]:
    name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void bhray::", "")
    blocks = int(r[grid_col]) // int(r[wg_col]) if wg_col else int(r[grid_col])
    groups.setdefault((name, blocks), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print("kernel | blocks | calls | median us | mean us | total ms")
for (name, blocks), v in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
    if len(v) >= 8:
        print(f"{name} | {blocks} | {len(v)} | {st.median(v):.1f} | {sum(v) / len(v):.1f} | {sum(v) / 1e3:.1f}")
