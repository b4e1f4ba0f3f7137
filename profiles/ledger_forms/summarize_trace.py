#!/usr/bin/env python
"""Per-launch view of the ledger's tick-side kernels in a rocprofv3 run of tools/assigned_probe.py (DESIGN.md §8g "Measured").

  rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d OUT -- python tools/assigned_probe.py --steps 6 [--records sink]
  python profiles/ledger_forms/summarize_trace.py OUT

The probe ticks context A (ledger) and context B (no ledger) in turn, so the even launches of k_expand_mapping are A's and the odd ones B's."""
import csv
import glob
import os
import sys

import numpy as np


def stat(name, v):
    v = np.asarray(v, float) / 1000.0
    if len(v):
        print(f"{name}: n={len(v)} p50={np.median(v):.2f} mean={v.mean():.2f} min={v.min():.2f} max={v.max():.2f} us; all: " + " ".join(f"{x:.1f}" for x in v))


def main(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    stat("k_insert", [dur for (_, dur, k) in rows if "k_insert" in k])  # (k_insert on the parent, k_insert_staged with the staging; the few-entry launches are redirects)
    em = [dur for (_, dur, k) in rows if "k_expand_mapping" in k]
    stat("k_expand_mapping all", em)
    stat("k_expand_mapping even launches (context A: ledger)", em[0::2])
    stat("k_expand_mapping odd launches (context B: no ledger)", em[1::2])
    for key in ("k_rel_claim", "k_rel_last_all", "k_rel_apply", "k_rel_rows", "select"):
        stat(key, [dur for (_, dur, k) in rows if key in k])
    for f in glob.glob(os.path.join(d, "**", "*_memory_copy_trace.csv"), recursive=True):
        g = {}
        for r in csv.DictReader(open(f)):
            g.setdefault(r.get("Direction", "?"), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        print("memory copies by direction: count, mean us, total us")
        for key, v in sorted(g.items(), key=lambda kv: -sum(kv[1])):
            print("  ", key, len(v), round(float(np.mean(v)) / 1000, 2), round(sum(v) / 1000, 1))


if __name__ == "__main__":
    main(sys.argv[1])
