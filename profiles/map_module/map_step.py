#!/usr/bin/env python
"""Once through every path of the mapping's host side (hqmap::Mapper), for a kernel trace: a dense tick, a tick on the ordered view, a tick with Retracting tasks
on each form, a prefill tick, a two-call tick with its replay (hqtick_ready_consume_last), a HQTICK_FLAG_CONSUME_IN_TICK tick, and one that fails on a record sink
too small and puts back what it took — on the dense scan and on the view.
Run from the repository root (the library of that tree is the one loaded).

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/map_module/map_step.py
  python profiles/cluster_module/launch_sequence.py OUT
"""
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.core import priority_from_user  # noqa: E402
from hyperqueue_amd.sharded import sink_layout  # noqa: E402
from hyperqueue_amd.tick import HqTickError, Tick  # noqa: E402

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
    kinds = [k for recs in r.records for (_t, _v, k) in recs]
    print(f"{what}: status {r.status}, {kinds.count(abi.HQ_REC_ASSIGN)} assigned, {kinds.count(abi.HQ_REC_PREFILL)} prefilled, {len(r.redirects)} redirects")


one, many = with_levels(1, 1), with_levels(4097, 3)

for what, cfg in (("fill_max 0", abi.make_config(reserve=0, fill_max=0, time_limit_s=20.0)), ("prefill", abi.make_config(reserve=0, fill_max=3, time_limit_s=20.0))):
    t = Tick(cfg)
    report(f"{what}: dense tick", t.tick(one))
    report(f"{what}: view tick", t.tick(many))
    report(f"{what}: retracting, dense", t.tick(with_retracting(with_levels(1, 5, n_classes=1))))
    report(f"{what}: retracting, view", t.tick(with_retracting(with_levels(4097, 6, n_classes=1))))
    for form, snap in (("dense", one), ("view", many)):  # the two-call form: the tick, then its selection once more as tombstones
        t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        report(f"{what}: two-call tick, {form}", t.tick(empty(snap), resident=True))
        t.ready_consume_last()
        print(f"{what}: consumed, {form}: {t.ready_count()} left")
        report(f"{what}: the next tick, {form}", t.tick(empty(snap), resident=True))
    t.close()

t = Tick(abi.make_config(reserve=0, fill_max=3, time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK))
small = torch.zeros(sink_layout(W, 2)[4], dtype=torch.uint8, device="cuda:0")
for form, snap in (("dense", one), ("view", many)):
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    report(f"consume-in-tick, {form}", t.tick(empty(snap), resident=True))
    print(f"consume-in-tick, {form}: {t.ready_count()} left")
    t.set_record_sink(small)
    try:
        t.tick(empty(snap), resident=True)
    except HqTickError as e:
        print(f"failed tick, {form}: {e}; {t.ready_count()} left")
    t.set_record_sink(None)
    report(f"after the restore, {form}", t.tick(empty(snap), resident=True))
    print(f"after the restore, {form}: {t.ready_count()} left")
t.close()
