#!/usr/bin/env python
"""One churn step on a resident worker set, for a kernel trace: a tick, hqtick_cluster_remove_workers of three workers, hqtick_cluster_add_workers of three, a tick.
Run from the repository root (the library of that tree is the one loaded); --ledger: with the assignment ledger on, whose steps interleave with the set's.

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/cluster_module/churn_step.py [--ledger]
  python profiles/cluster_module/launch_sequence.py OUT
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402

ledger = "--ledger" in sys.argv
snap = workloads.make("c3", n_tasks=20_000, n_workers=64)
t = Tick(abi.make_config(time_limit_s=20.0))
t.cluster_upload(snap)
if ledger:
    t.assigned_enable([])


def tick():
    sc = snap.to_c(resident_workers=True)
    if ledger:
        sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    return t.tick_raw(sc)


tick()
t.cluster_remove_workers(snap.worker_id[[3, 17, 40]])
row = np.asarray(snap.worker_total, np.uint64).reshape(64, -1)[:1]
t.cluster_add_workers([1001, 1002, 1003], np.tile(row, (3, 1)))
r = tick()
print("status", r.status, "records", int(np.ctypeslib.as_array(r.rec_off, shape=(65,))[64]))
t.close()
