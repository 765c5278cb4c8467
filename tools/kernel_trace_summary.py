#!/usr/bin/env python3
"""Per kernel of a rocprofv3 --kernel-trace CSV: dispatches, mean duration, registers, LDS and scratch as the runtime launched it.
usage: kernel_trace_summary.py <dir with *kernel_trace.csv> <out.csv>"""
import csv
import glob
import os
import sys
from collections import defaultdict

src, out = sys.argv[1], sys.argv[2]
agg = defaultdict(lambda: [0, 0.0, None])
for f in glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True):
    with open(f, newline="") as fh:
        for row in csv.DictReader(fh):
            a = agg[row["Kernel_Name"].split("(")[0][:80]]
            a[0] += 1
            a[1] += (float(row["End_Timestamp"]) - float(row["Start_Timestamp"])) / 1e6
            a[2] = tuple(row.get(k, "") for k in ("VGPR_Count", "Accum_VGPR_Count", "SGPR_Count", "LDS_Block_Size", "Scratch_Size", "Workgroup_Size", "Grid_Size"))
with open(out, "w", newline="") as fh:
    w = csv.writer(fh)
    w.writerow(["Kernel_Name", "Dispatches", "Mean_ms", "VGPR_Count", "Accum_VGPR_Count", "SGPR_Count", "LDS_Block_Size", "Scratch_Size", "Workgroup_Size", "Grid_Size"])
    for k, (n, ms, r) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        w.writerow([k, n, f"{ms / n:.4f}", *r])
