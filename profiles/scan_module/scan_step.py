#!/usr/bin/env python
"""Once through every path of phase A (hqscan::Scanner), for a kernel trace: a first dense tick (the speculative scan), a tick on the cached level table, a 5-level
tick (the speculative scan refuses, the second attempt runs), a tick over the level cap into the ordered view, a tick back under the cap (the view once more, then
the dense scan), ticks with Retracting tasks on the dense scan and on the view, hqtick_query_resident on the census and beyond its caps.
Run from the repository root (the library of that tree is the one loaded).

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/scan_module/scan_step.py
  python profiles/cluster_module/launch_sequence.py OUT
"""
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.core import priority_from_user  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402

N, W = 4200, 8


def with_levels(n_levels: int, seed: int, n_classes: int = 2) -> abi.Snapshot:
    """c3's cluster at 8 workers of 1/16 of their cpus and a ready set of N tasks in which every one of n_levels user priorities occurs, over n_classes requests"""
    snap = workloads.make("c3", seed=seed, n_tasks=N, n_workers=W)
    rng = np.random.default_rng(seed)
    snap.requests = [[workloads._variant([(0, 1 + (q % 4))])] for q in range(n_classes)]
    snap.task_rq = rng.integers(0, n_classes, N).astype(np.uint32)
    lv = np.concatenate([np.arange(n_levels), rng.integers(0, n_levels, N - n_levels)])
    rng.shuffle(lv)
    snap.task_priority = np.asarray([priority_from_user(int(p)) for p in lv], np.uint64)
    snap.worker_total = snap.worker_total.copy()
    snap.worker_total[:, 0] //= 16
    snap.worker_free = snap.worker_total.copy()
    return snap


def with_retracting(snap: abi.Snapshot) -> abi.Snapshot:
    order = np.lexsort((snap.task_id, ~snap.task_priority))  # the queues' take order: three that a tick takes, two out of its reach (prefill sets included)
    pick = np.sort(snap.task_id[order[[0, 5, 17, 4000, 4100]]])
    return dataclasses.replace(snap, _keep=[], retracting=[(int(tid), i % W, abi.HQ_NO_WORKER, 0) for i, tid in enumerate(pick.tolist())])


def empty(snap: abi.Snapshot) -> abi.Snapshot:
    return dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))


def report(what: str, r: abi.Result):
    print(f"{what}: status {r.status}, {sum(len(w) for w in r.records)} records, {len(r.redirects)} redirects")


one, five, many, three = with_levels(1, 1), with_levels(5, 2), with_levels(4097, 3), with_levels(3, 4)
t = Tick(abi.make_config(time_limit_s=20.0))


def resident_tick(what: str, snap: abi.Snapshot, consume: bool = True):
    report(what, t.tick(empty(snap), resident=True))
    if consume:
        t.ready_consume_last()


t.upload_ready(one.task_id, one.task_priority, one.task_rq)
resident_tick("first dense tick", one)
resident_tick("cached level table", one)
t.upload_ready(five.task_id, five.task_priority, five.task_rq)
resident_tick("five levels", five)
t.upload_ready(many.task_id, many.task_priority, many.task_rq)
resident_tick("over the level cap", many)
t.upload_ready(three.task_id, three.task_priority, three.task_rq)
resident_tick("back under the cap, on the view", three)
resident_tick("back under the cap, dense", three)
report("retracting, dense", t.tick(with_retracting(with_levels(1, 5, n_classes=1))))
report("retracting, view", t.tick(with_retracting(with_levels(4097, 6, n_classes=1))))
fake_ids = np.arange(1 << 20, (1 << 20) + 3, dtype=np.uint32)
fake_total = np.zeros((3, one.n_resources), np.uint64); fake_total[:, 0] = 16 * abi.HQ_FRACTIONS_PER_UNIT
for what, snap in (("census", five), ("census beyond the caps", many)):
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    loaded, optimal, rq_ready = t.query_resident(empty(snap), fake_ids, fake_total)
    print(f"{what}: loaded {loaded.astype(int).tolist()}, optimal {optimal}, rq_ready {rq_ready.tolist()}")
t.close()
