"""hqtick_finish_tasks at c3p scale against today's sequence on the same context and build.

State: the c3p steady workload (1 M tasks, 1024 workers) with every task in the dependency graph, the ledger and prefilled tracking on, one tick consumed.
Two batches of (id, reporting worker) pairs, every pair rightly reported, in alternating rounds with the state restored (outside the timed part) before every
timed call:
  some    1000 of the tick's assigned ids
  all     every assigned id of the tick, shuffled
The yardstick is what a host does today for the same handler: hqtick_graph_finish(ids) + hqtick_assigned_release(ids).  Prints one JSON line: per-call p50 wall
time of both with the min and max of the rounds (the spread), and the bytes either moves over PCIe (computed from the call's arguments and answers).

    python tools/finish_probe.py [--reps 5] [--tasks 1000000] [--workers 1024] [--only some|all]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--workers", type=int, default=1024)
    ap.add_argument("--only", choices=["some", "all"], default=None)
    args = ap.parse_args()
    snap = workloads.make_steady("c3p", seed=3, n_tasks=args.tasks, n_workers=args.workers)
    W, R = len(snap.worker_id), snap.n_resources
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    ids, prio, rqs = np.asarray(snap.task_id, np.uint64), np.asarray(snap.task_priority, np.uint64), np.asarray(snap.task_rq, np.uint32)
    assert (ids[1:] > ids[:-1]).all()
    meta = {int(t): (int(p), int(q)) for t, p, q in zip(ids, prio, rqs)}
    t = Tick(abi.make_config(time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK | abi.HQTICK_FLAG_NO_KERNEL_TIMING))
    t.cluster_upload(snap)
    t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    no_deps = (np.zeros(len(ids) + 1, np.uint32), np.zeros(0, np.uint64))
    assert len(t.graph_add_tasks(ids, prio, rqs, no_deps)) == len(ids)
    t.assigned_enable([]); t.assigned_track_prefilled([])
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None; sc.prefilled_off = None; sc.prefilled_rq = None
    res = abi.parse_result(t.tick_raw(sc, resident=True), W, R)
    wid = snap.worker_id.tolist()
    asg = {tid: (tid, wid[w], meta[tid][1], v, meta[tid][0]) for w, recs in enumerate(res.records) for (tid, v, k) in recs if k == abi.HQ_REC_ASSIGN}
    assert t.assigned_count() == len(asg)
    state0 = (t.ready_count(), t.assigned_count(), t.assigned_prefilled_count(), t.assigned_free_rows().copy())

    rng = np.random.default_rng(5)
    a_ids = np.asarray(sorted(asg), np.uint64)
    everything = a_ids.copy(); rng.shuffle(everything)
    batches = {"some": rng.choice(a_ids, min(1000, len(a_ids)), replace=False), "all": everything}
    if args.only:
        batches = {args.only: batches[args.only]}

    def restore(batch):
        gone = np.sort(batch)
        at = np.searchsorted(ids, gone)
        t.graph_add_tasks(gone, prio[at], rqs[at], (np.zeros(len(gone) + 1, np.uint32), np.zeros(0, np.uint64)))
        t.ready_remove(gone)
        assert t.assigned_add([asg[x] for x in gone.tolist()]) == len(gone)
        now = (t.ready_count(), t.assigned_count(), t.assigned_prefilled_count(), t.assigned_free_rows())
        assert now[:3] == state0[:3] and (now[3] == state0[3]).all(), "the state was not restored"

    def todays(batch):
        rel, unknown = t.graph_finish(batch)
        return t.assigned_release(batch), rel, unknown

    out = {"tasks": len(ids), "workers": W, "assigned": len(asg), "reps": args.reps}
    for name, batch in batches.items():
        reporters = np.asarray([asg[x][1] for x in batch.tolist()], np.uint32)
        t_new, t_old, got = [], [], None
        for rep in range(args.reps):
            if rep:
                restore(batch)
            t0 = time.perf_counter(); got = t.finish_tasks(batch, reporters); t_new.append(time.perf_counter() - t0)
            after_new = (t.ready_count(), t.assigned_count(), t.assigned_free_rows().copy())
            restore(batch)
            t0 = time.perf_counter(); done, rel, unknown = todays(batch); t_old.append(time.perf_counter() - t0)
            after_old = (t.ready_count(), t.assigned_count(), t.assigned_free_rows())
            assert after_new[:2] == after_old[:2] and (after_new[2] == after_old[2]).all()
            assert got["accepted"] == done == len(batch) and unknown == 0 and (rel == got["released"]).all()
        restore(batch)
        n, c = len(batch), len(got["released"])
        us = lambda x: [round(float(v) * 1e6, 1) for v in (np.median(x), np.min(x), np.max(x))]  # noqa: E731
        out[name] = {"ids": n, "released": c, "finish_call_us_p50_min_max": us(t_new), "todays_sequence_us_p50_min_max": us(t_old),
                     "todays_over_finish": round(float(np.median(t_old) / np.median(t_new)), 2),
                     # up: ids + reporters once / the ids twice; down: the kinds, the ledger's counters, the graph's counters and released ids /
                     # two sets of counters and the released ids
                     "pcie_bytes_finish": 12 * n + n + 32 + 64 + 8 * c, "pcie_bytes_todays": 2 * 8 * n + 32 + 64 + 8 * c}
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
