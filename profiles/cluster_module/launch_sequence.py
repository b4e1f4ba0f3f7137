#!/usr/bin/env python
"""Every kernel launch of a rocprofv3 --kernel-trace run in time order, as `kernel:grid:workgroup` (two runs with the same output launched the same kernels)."""
import csv
import glob
import os
import re
import sys

rows = []
for f in glob.glob(os.path.join(sys.argv[1], "**", "*_kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        m = re.search(r"(k_\w+)", r["Kernel_Name"])
        rows.append((int(r["Start_Timestamp"]), m.group(1) if m else r["Kernel_Name"], r["Grid_Size_X"], r["Workgroup_Size_X"]))
rows.sort()
print(len(rows), "launches")
print("\n".join(f"{k}:{g}:{w}" for (_, k, g, w) in rows))
