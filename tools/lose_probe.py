"""hqtick_lose_workers at c3p scale, with the protocol of tools/reject_probe.py: one MI355X, the c3p steady workload (1 M tasks, 1024 workers) in
the dependency graph, ledger and prefilled tracking on, one tick consumed.  Batches of 1, 4, 16 and 128 lost workers (drawn once, shuffled).  Every batch is timed
in three forms that alternate round by round on the same context, the C call alone (no list is copied into Python inside the timed part):
    new            hqtick_lose_workers(list)
    parent         hqtick_cluster_remove_workers(list)
    parent_each    one hqtick_cluster_remove_workers call per worker: what a host that needs per-worker running lists has to do today (batches of more than one)
The state is restored (outside the timed part) after every timed call: the lost workers join again under fresh ids (ids only ascend) with their total rows,
their assigned entries enter again (hqtick_assigned_add), the prefilled entries are seeded again, the requeued ids leave the ready set.  Rows therefore move; the
forms are compared by the workers' original positions.  The probe stops if two forms leave different ledger counts, free rows or ready count.  Prints one JSON
line: per batch the p50 wall time of each form with the min and max of the rounds.  Host waits per hqtick_lose_workers call: DESIGN.md §8n.

    python tools/lose_probe.py [--reps 7] [--tasks 1000000] [--workers 1024]
"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--workers", type=int, default=1024)
    args = ap.parse_args()
    snap = workloads.make_steady("c3p", seed=3, n_tasks=args.tasks, n_workers=args.workers)
    W, R = len(snap.worker_id), snap.n_resources
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    ids, prio, rqs = np.asarray(snap.task_id, np.uint64), np.asarray(snap.task_priority, np.uint64), np.asarray(snap.task_rq, np.uint32)
    t = Tick(abi.make_config(time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK | abi.HQTICK_FLAG_NO_KERNEL_TIMING))
    t.cluster_upload(snap)
    t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert len(t.graph_add_tasks(ids, prio, rqs, (np.zeros(len(ids) + 1, np.uint32), np.zeros(0, np.uint64)))) == len(ids)
    t.assigned_enable([]); t.assigned_track_prefilled([])
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None; sc.prefilled_off = None; sc.prefilled_rq = None
    res = abi.parse_result(t.tick_raw(sc, resident=True), W, R)
    assert not res.mn
    where = {int(x): k for k, x in enumerate(ids.tolist())}
    rq_of = lambda x: int(rqs[where[x]])  # noqa: E731
    pr_of = lambda x: int(prio[where[x]])  # noqa: E731
    total = np.asarray(snap.worker_total, np.uint64).reshape(W, R)
    cur = snap.worker_id.tolist()  # original position -> the id the worker has now
    next_id = max(cur) + 1
    asg = [[(tid, v) for (tid, v, k) in recs if k == abi.HQ_REC_ASSIGN] for recs in res.records]
    pf = [[tid for (tid, v, k) in recs if k == abi.HQ_REC_PREFILL] for recs in res.records]
    n_asg, n_pf, n_ready = sum(map(len, asg)), sum(map(len, pf)), t.ready_count()
    assert t.assigned_count() == n_asg and t.assigned_prefilled_count() == n_pf

    def state():
        pos = {w: k for k, w in enumerate(t.cluster_workers().tolist())}
        rows = t.assigned_free_rows()
        keep = [p for p in range(W) if cur[p] in pos]
        return (t.assigned_count(), t.assigned_prefilled_count(), t.ready_count(), tuple(keep), rows[[pos[cur[p]] for p in keep]].tobytes())

    lib = t._lib
    lib.hqtick_lose_workers.argtypes = [C.c_void_p, C.c_uint32, abi.u32p]
    lib.hqtick_cluster_remove_workers.argtypes = [C.c_void_p, C.c_uint32, abi.u32p]
    order = np.random.default_rng(5).permutation(W)
    out = {"tasks": len(ids), "workers": W, "assigned": n_asg, "prefilled": n_pf, "ready": n_ready, "reps": args.reps}
    for n in (1, 4, 16, 128):
        if n * 2 > W:
            continue
        batch = [int(p) for p in order[:n]]  # original positions
        held = sorted([x for p in batch for (x, _) in asg[p]] + [x for p in batch for x in pf[p]])
        s_id = np.asarray(held, np.uint64)

        def restore():
            nonlocal next_id
            fresh = list(range(next_id, next_id + n)); next_id += n
            t.cluster_add_workers(fresh, total[batch], total[batch])
            for p, w in zip(batch, fresh):
                cur[p] = w
            entries = [(x, cur[p], rq_of(x), v, pr_of(x)) for p in batch for (x, v) in asg[p]]
            assert t.assigned_add(entries) == len(entries)
            seeds = [(x, cur[p], rq_of(x), pr_of(x)) for p in range(W) for x in pf[p]]
            assert t.assigned_track_prefilled(seeds) == len(seeds)
            assert t.ready_remove(s_id) == len(held)
            assert t.assigned_count() == n_asg and t.assigned_prefilled_count() == n_pf and t.ready_count() == n_ready, "not restored"

        def timed(form):
            arr = np.asarray([cur[p] for p in batch], np.uint32)
            ptr = arr.ctypes.data_as(abi.u32p)
            t0 = time.perf_counter()
            if form == "new":
                rc = lib.hqtick_lose_workers(t._ctx, n, ptr)
            elif form == "parent":
                rc = lib.hqtick_cluster_remove_workers(t._ctx, n, ptr)
            else:
                rc = 0
                for k in range(n):
                    rc = min(rc, lib.hqtick_cluster_remove_workers(t._ctx, 1, arr[k:k + 1].ctypes.data_as(abi.u32p)))
            dt = time.perf_counter() - t0
            assert rc >= 0, (form, rc, t._err())
            return dt

        forms = ["new", "parent"] + (["parent_each"] if n > 1 else [])
        times = {f: [] for f in forms}
        for rep in range(args.reps + 1):  # (the first round allocates the calls' buffers: not timed)
            after = None
            for f in forms:
                dt = timed(f)
                if rep:
                    times[f].append(dt)
                if f == "new":
                    assert [x[0] for x in t.lose_last()["requeued"]] == held
                s = state()
                assert after is None or s == after, f"{f} leaves another state than hqtick_lose_workers"
                after = s
                restore()
        us = lambda x: [round(float(v) * 1e6, 1) for v in (np.median(x), np.min(x), np.max(x))]  # noqa: E731
        out[f"lost_{n}"] = {"workers": n, "entries": len(held), **{f + "_us_p50_min_max": us(times[f]) for f in forms},
                            "ratio_new_over_parent": round(float(np.median(times["new"]) / np.median(times["parent"])), 3)}
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
