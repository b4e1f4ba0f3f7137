#!/usr/bin/env python
"""Every delta of the resident ready set once, for a kernel trace: upload, tick + consume, a packed batch appended, a batch merged, a batch appended behind the merge,
a remove, a compaction, tick + consume; then a first batch onto an empty set and one behind it.  Run from the root of the tree whose library is to be loaded.

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/ready_set/delta_step.py
  python profiles/cluster_module/launch_sequence.py OUT
"""
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402

snap = workloads.make("c3", n_tasks=20_000, n_workers=24)
empty = dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))
p0, top = int(snap.task_priority[0]), int(snap.task_id[-1])
t = Tick(abi.make_config(time_limit_s=20.0))
t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)


def tick():
    r = t.tick(empty, resident=True)
    t.ready_consume_last()
    return sum(len(x) for x in r.records)


def batch(first, n):
    return np.uint64(first) + np.arange(n, dtype=np.uint64), np.full(n, p0, np.uint64), (np.arange(n) % 8).astype(np.uint32)


placed = [tick()]
t.ready_add_packed([(top + 1, 1000)], [(p0, 1000)], (np.arange(1000) % 8).astype(np.uint16))  # fresh ids, room in the upload's slack: appended
t.ready_add(*batch(1, 500))                                                                    # ids below everything resident: merged
t.ready_add(*batch(top + 1001, 3000))                                                          # fresh ids behind the merge's room: appended
assert t.ready_remove(snap.task_id[-200:]) == 200
t.ready_compact()
placed.append(tick())
count, appends = t.ready_count(), t.kernel_stats()["ready_appends"]
t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
t.ready_add(*batch(1, 64))    # the first batch becomes the set
t.ready_add(*batch(65, 4))    # ... and leaves room: appended
print("placed", placed, "ready_count", count, "then", t.ready_count(), "ready_appends", appends, "then", t.kernel_stats()["ready_appends"])
t.close()
