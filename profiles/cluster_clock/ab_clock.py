#!/usr/bin/env python
"""Tick time of a cluster of identical time-limited workers with distinct deadlines, on the two protocols (profiles/cluster_clock/README.md).

    python profiles/cluster_clock/ab_clock.py --mode rows|clock [--workload c3p] [--steps 200] [--warmup 20]

rows:  the row-delta protocol — before every tick all W rows go to hqtick_cluster_update_workers with their free resources and true remaining lifetimes.
clock: hqtick_cluster_set_clock alone.
Run from the root of the tree to measure (the commit before clock mode can only run `rows`).  Cold ticks on the resident ready set, as bench.py's headline: the
ready set and the free rows do not change, only the time passes (1 ms per tick).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["rows", "clock"], required=True)
ap.add_argument("--workload", default="c3p")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()

snap = workloads.make(args.workload, seed=0)
W, R = len(snap.worker_id), snap.n_resources
now = 1_000_000_000_000
term = now + 3_600_000_000_000 + np.arange(W, dtype=np.int64) * 1_000  # an hour of lifetime, connected a microsecond apart: beyond every threshold
snap.worker_remaining_ns = (term - now).astype(np.int64)
t = Tick(abi.make_config(time_limit_s=20.0))
t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
t.cluster_upload(snap)
sc = snap.to_c(resident_workers=True)
lib, ctx = t._lib, t._ctx
idx = np.arange(W, dtype=np.uint32); free = np.ascontiguousarray(snap.worker_free, np.uint64).reshape(-1); rem = np.empty(W, np.int64)
lib.hqtick_cluster_update_workers.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
if args.mode == "clock":
    lib.hqtick_cluster_set_clock.argtypes = [C.c_void_p, C.c_int64]
    assert lib.hqtick_cluster_set_clock(ctx, now) == 0
out = abi.ResultC()
lat, model_us = [], []
for i in range(args.warmup + args.steps):
    now += 1_000_000
    a = time.perf_counter()
    if args.mode == "clock":
        rc = lib.hqtick_cluster_set_clock(ctx, now)
    else:
        np.subtract(term, now, out=rem)  # (the host's own bookkeeping of W lifetimes is part of this protocol)
        rc = lib.hqtick_cluster_update_workers(ctx, W, idx.ctypes.data, free.ctypes.data, rem.ctypes.data)
    rc2 = lib.hqtick_run_resident(ctx, C.byref(sc), C.byref(out))
    b = time.perf_counter()
    assert rc == 0 and rc2 >= 0, (rc, rc2, t._err())
    if i >= args.warmup:
        lat.append((b - a) * 1e3); model_us.append(t.kernel_stats()["model_us"])
groups = t.cluster_last_row_groups() if hasattr(t, "cluster_last_row_groups") else None
n_rec = int(out.rec_off[W]) if out.rec_off else None
print(json.dumps({"mode": args.mode, "workload": args.workload, "W": W, "steps": args.steps, "p50_ms": round(float(np.percentile(lat, 50)), 4), "p10_ms": round(float(np.percentile(lat, 10)), 4),
                  "p90_ms": round(float(np.percentile(lat, 90)), 4), "mean_ms": round(float(np.mean(lat)), 4), "model_us_p50": round(float(np.percentile(model_us, 50)), 1),
                  "row_groups": groups, "status": int(out.status), "n_records": n_rec}))
t.close()
