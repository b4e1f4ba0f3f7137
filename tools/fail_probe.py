"""hqtick_fail_tasks at c3p scale against the parent's sequence on the same context and build.

State: the c3p steady workload (1 M tasks, 1024 workers) with every task in the dependency graph, the ledger and prefilled tracking on, and beside it 256 failing
roots, each assigned on a worker of its own and each with a closure of 64 consumers two levels deep (8 children, 7 grandchildren under each child).  One batch of
k rightly reported roots for k in {1, 16, 256}, in alternating rounds with the state restored (outside the timed part) before every timed call.  The yardstick is
what a host does at the parent commit for the same k Failed updates: one hqtick_assigned_release(ids) and, to learn each task's own consumers, k
hqtick_graph_remove([id], 1) calls, each followed by hqtick_ready_remove of what it removed.  Prints one JSON line: per-call p50 wall time of both with the min and
max of the rounds.

    python tools/fail_probe.py [--reps 5] [--tasks 1000000] [--workers 1024] [--k 1,16,256] [--only new|old]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402

ROOTS, CHILDREN, GRAND = 256, 8, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--workers", type=int, default=1024)
    ap.add_argument("--k", default="1,16,256")
    ap.add_argument("--only", choices=["new", "old"], default=None)
    args = ap.parse_args()
    snap = workloads.make_steady("c3p", seed=3, n_tasks=args.tasks, n_workers=args.workers)
    W = len(snap.worker_id)
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    ids, prio, rqs = np.asarray(snap.task_id, np.uint64), np.asarray(snap.task_priority, np.uint64), np.asarray(snap.task_rq, np.uint32)
    t = Tick(abi.make_config(time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK | abi.HQTICK_FLAG_NO_KERNEL_TIMING))
    t.cluster_upload(snap)
    t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert len(t.graph_add_tasks(ids, prio, rqs, (np.zeros(len(ids) + 1, np.uint32), np.zeros(0, np.uint64)))) == len(ids)
    t.assigned_enable([]); t.assigned_track_prefilled([])

    # the failing part: root r, its children, their grandchildren, ids above the workload's
    per = 1 + CHILDREN + CHILDREN * GRAND
    base = int(ids.max()) + 1
    wid = snap.worker_id.tolist()
    rq0, prio0 = int(rqs[0]), int(prio[0])

    def family(r):
        """(ids, deps) of root r's family, ids ascending: the root, the children, the grandchildren"""
        b = base + r * per
        f_ids = list(range(b, b + per))
        deps = [[]] + [[b]] * CHILDREN + [[b + 1 + g // GRAND] for g in range(CHILDREN * GRAND)]
        return f_ids, deps

    def enter(roots):
        f_ids, deps = [], []
        for r in roots:
            a, d = family(r)
            f_ids += a; deps += d
        now = t.graph_add_tasks(f_ids, [prio0] * len(f_ids), [rq0] * len(f_ids), deps)
        assert len(now) == len(roots)
        t.ready_remove(now)  # the roots are held, not queued
        assert t.assigned_add([(base + r * per, wid[r % W], rq0, 0, prio0) for r in roots]) == len(roots)

    enter(range(ROOTS))
    state0 = (t.ready_count(), t.assigned_count(), t.graph_stats()["n_tasks"], t.assigned_free_rows().copy())

    def restored():
        now = (t.ready_count(), t.assigned_count(), t.graph_stats()["n_tasks"], t.assigned_free_rows())
        assert now[:3] == state0[:3] and (now[3] == state0[3]).all(), "the state was not restored"

    def parents(batch):
        done = t.assigned_release(batch)
        lists = []
        for x in batch.tolist():
            rem = t.graph_remove([x], True)
            t.ready_remove(rem)
            lists.append(rem[rem != x])
        return done, lists

    out = {"tasks": len(ids) + ROOTS * per, "workers": W, "closure_per_root": per - 1, "reps": args.reps}
    for k in [int(x) for x in args.k.split(",")]:
        roots = list(range(k))
        batch = np.asarray([base + r * per for r in roots], np.uint64)
        reporters = np.asarray([wid[r % W] for r in roots], np.uint32)
        t_new, t_old, got, lists = [], [], None, None
        for rep in range(args.reps + 1):  # (the first round allocates the call's staging: not timed)
            if args.only != "old":
                t0 = time.perf_counter(); got = t.fail_tasks(batch, reporters); dt = time.perf_counter() - t0
                if rep:
                    t_new.append(dt)
                assert got["accepted"] == k and len(got["consumer_id"]) == k * (per - 1) and int(got["consumer_off"][1]) == per - 1
                enter(roots); restored()
            if args.only != "new":
                t0 = time.perf_counter(); done, lists = parents(batch); dt = time.perf_counter() - t0
                if rep:
                    t_old.append(dt)
                assert done == k and all(len(x) == per - 1 for x in lists)
                if got is not None:
                    assert (np.concatenate(lists) == got["consumer_id"]).all()
                enter(roots); restored()
        us = lambda x: [round(float(v) * 1e6, 1) for v in (np.median(x), np.min(x), np.max(x))] if x else None  # noqa: E731
        out["k%d" % k] = {"roots": k, "removed": k * per, "fail_call_us_p50_min_max": us(t_new), "parents_sequence_us_p50_min_max": us(t_old),
                          "parents_over_fail": round(float(np.median(t_old) / np.median(t_new)), 2) if t_new and t_old else None}
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
