#!/usr/bin/env python
"""The ledger's kernels (namespace hqasg) in a rocprofv3 run of tools/assigned_probe.py: per kernel and grid the launches and durations, and per release the
sum of its four kernels (prefilled tasks).

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/assigned_probe.py --steps 6 [--prefill]
  python profiles/ledger_prefill/summarize_trace.py OUT
"""
import collections
import csv
import glob
import os
import re
import sys

import numpy as np


def short(name):
    m = re.search(r"(k_\w+)", name)
    return m.group(1) if m else name


def main(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "hqasg" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), short(r["Kernel_Name"]), int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"])))
    rows.sort()
    by = collections.defaultdict(list)
    for (_, dur, k, grid, wg) in rows:
        by[(k, grid, wg)].append(dur / 1000.0)
    print("kernel grid workgroup launches p50_us mean_us min_us max_us")
    for (k, grid, wg), v in sorted(by.items()):
        print(f"{k} {grid} {wg} {len(v)} {np.median(v):.2f} {np.mean(v):.2f} {min(v):.2f} {max(v):.2f}")
    rel = [r for r in rows if r[2].startswith("k_rel_")]
    sums = [sum(x[1] for x in rel[i:i + 4]) / 1000.0 for i in range(0, len(rel) - 3, 4)]
    if sums and [x[2] for x in rel[:4]] == ["k_rel_claim", "k_rel_last_all", "k_rel_apply", "k_rel_rows"]:
        print(f"release (sum of its four kernels) n={len(sums)} p50={np.median(sums):.2f} mean={np.mean(sums):.2f} us; all: " + " ".join(f"{x:.1f}" for x in sums))
    print("launch sequence: " + " ".join(f"{k}:{grid}" for (_, _, k, grid, _) in rows))
    ins = [(grid, dur / 1000.0) for (_, dur, k, grid, _) in rows if k == "k_insert_staged"]
    if ins:  # (the grid is the record count rounded up to 256 threads)
        print("k_insert_staged ns per record (grid threads): " + " ".join(f"{1000.0 * d / g:.3f}" for g, d in ins) + f"; p50 {np.median([1000.0 * d / g for g, d in ins]):.3f}")


if __name__ == "__main__":
    main(sys.argv[1])
