"""hqtick_cancel_tasks at c3p scale against today's sequence on the same context and build.

State: the c3p steady workload (1 M tasks, 1024 workers) with every task in the dependency graph, the ledger and prefilled tracking on, one tick consumed.
Two batches, in alternating rounds with the state restored (outside the timed part) before every timed call:
  mixed   1000 ids: 400 assigned, 100 prefilled (as many as the tick made), 400 ready, 50 unknown, 50 repeats
  all     every id of the workload
The yardstick is what a host does today for the same handler: hqtick_assigned_lookup + grouping on the host (numpy: first mention of an id, stable sort by
worker) for the CancelTasks lists, then hqtick_graph_remove(ids, 1) + hqtick_assigned_release + hqtick_assigned_unprefill.  Prints one JSON line: per-call p50
wall time of both, the bytes either moves over PCIe (computed from the call's arguments and answers), and the sizes of the answers.

    python tools/cancel_probe.py [--reps 7] [--tasks 1000000] [--workers 1024] [--only mixed|all]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--workers", type=int, default=1024)
    ap.add_argument("--only", choices=["mixed", "all"], default=None)
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
    pf = {tid: (tid, wid[w], meta[tid][1], meta[tid][0]) for w, recs in enumerate(res.records) for (tid, v, k) in recs if k == abi.HQ_REC_PREFILL}
    assert t.assigned_count() == len(asg) and t.assigned_prefilled_count() == len(pf)
    placed = set(asg) | set(pf)
    placed_ids = np.asarray(sorted(placed), np.uint64)
    ready = np.asarray([x for x in ids.tolist() if x not in placed], np.uint64)
    state0 = (t.ready_count(), t.assigned_count(), t.assigned_prefilled_count(), t.assigned_free_rows().copy())

    rng = np.random.default_rng(5)
    a_ids, p_ids = np.asarray(sorted(asg), np.uint64), np.asarray(sorted(pf), np.uint64)
    mixed = np.concatenate([rng.choice(a_ids, min(400, len(a_ids)), replace=False), rng.choice(p_ids, min(100, len(p_ids)), replace=False), rng.choice(ready, 400, replace=False),
                            np.arange(50, dtype=np.uint64) + (1 << 50)])
    mixed = np.concatenate([mixed, rng.choice(mixed[:400], 50, replace=False)])
    rng.shuffle(mixed)
    batches = {"mixed": mixed, "all": ids.copy()}
    if args.only:
        batches = {args.only: batches[args.only]}

    def restore(batch):
        gone = np.unique(batch[np.isin(batch, ids)])
        at = np.searchsorted(ids, gone)
        t.graph_add_tasks(gone, prio[at], rqs[at], (np.zeros(len(gone) + 1, np.uint32), np.zeros(0, np.uint64)))
        back = gone[np.isin(gone, placed_ids)]
        if len(back):
            t.ready_remove(back)
        add = [asg[x] for x in back.tolist() if x in asg]
        if add:
            assert t.assigned_add(add) == len(add)
        assert t.assigned_track_prefilled(list(pf.values())) == len(pf)
        now = (t.ready_count(), t.assigned_count(), t.assigned_prefilled_count(), t.assigned_free_rows())
        assert now[:3] == state0[:3] and (now[3] == state0[3]).all(), "the state was not restored"

    def todays(batch):
        lw, _ = t.assigned_lookup(batch)
        first = np.zeros(len(batch), bool); first[np.unique(batch, return_index=True)[1]] = True
        pos = np.flatnonzero(first & (lw != abi.HQ_NO_WORKER))
        order = pos[np.argsort(lw[pos], kind="stable")]
        workers, counts = np.unique(lw[pos], return_counts=True)
        lists = (workers, np.concatenate([[0], np.cumsum(counts)]), batch[order])
        closure = t.graph_remove(batch, recursive=True)
        t.assigned_release(batch); t.assigned_unprefill(batch)
        return lists, closure

    out = {"tasks": len(ids), "workers": W, "assigned": len(asg), "prefilled": len(pf), "reps": args.reps}
    for name, batch in batches.items():
        t_new, t_old, got, lists = [], [], None, None
        for rep in range(args.reps):
            if rep:
                restore(batch)
            t0 = time.perf_counter(); got = t.cancel_tasks(batch, as_csr=True); t_new.append(time.perf_counter() - t0)
            after_new = (t.ready_count(), t.assigned_count(), t.assigned_prefilled_count(), t.assigned_free_rows().copy())
            restore(batch)
            t0 = time.perf_counter(); lists, closure = todays(batch); t_old.append(time.perf_counter() - t0)
            after_old = (t.ready_count(), t.assigned_count(), t.assigned_prefilled_count(), t.assigned_free_rows())
            assert after_new[:3] == after_old[:3] and (after_new[3] == after_old[3]).all() and (closure == got["closure"]).all()
            assert (got["messages"][0] == lists[0]).all() and (got["messages"][1] == lists[1]).all() and (got["messages"][2] == lists[2]).all()
        restore(batch)
        n, m, c = len(batch), got["n_ids"], len(got["closure"])
        p50 = lambda x: round(float(np.median(x)) * 1e6, 1)  # noqa: E731
        out[name] = {"ids": n, "ids_in_messages": m, "workers_told": len(got["messages"][0]), "closure": c, "ready_removed": got["ready_removed"],
                     "cancel_call_us_p50": p50(t_new), "todays_sequence_us_p50": p50(t_old), "todays_over_cancel": round(float(np.median(t_old) / np.median(t_new)), 2),
                     # up: the ids (once / four times); down: closure ids, then lists + routes + counters / lookup columns + three sets of counters
                     "pcie_bytes_cancel": 8 * n + 8 * c + (8 * m + 4 * (2 * len(got["messages"][0]) + 1) + 5 * n + 8 + 32),
                     "pcie_bytes_todays": 4 * 8 * n + 8 * c + (5 * n + 3 * 32)}
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
