"""hqtick_reject_tasks at c3p scale, with the protocol of tools/start_probe.py: one MI355X, the c3p steady workload (1 M tasks, 1024 workers) in
the dependency graph, ledger and prefilled tracking on, one tick consumed.  Batches of k = 1, 16, 256 and 4096 of the tick's assigned ids (shuffled), and one of all
of the tick's prefilled ids.  Every batch is timed in two forms that alternate round by round on the same context:
    new      hqtick_reject_tasks(ids, workers, variants)
    parent   the sequence a ledger host had to drive before: hqtick_assigned_release (hqtick_assigned_unprefill for the prefilled batch), hqtick_ready_add of the
             ids sorted with their requests and priorities, and hqtick_cluster_set_blocked with the whole list of every worker of the batch (the lists are
             built outside the timed part: keeping them is the host's own cost)
The state is restored (outside the timed part) after every timed call: the ids leave the ready set, the entries enter again, the blocked sets are emptied.  Both
forms must leave the same ledger counts, free rows, ready count and blocked pairs.  Prints one JSON line: per batch the p50 wall time of each form with the min and
max of the rounds, and the ratio of the medians.  Host waits per hqtick_reject_tasks call: one behind the ledger's passes, one in the ready set's merge.

    python tools/reject_probe.py [--reps 7] [--tasks 1000000] [--workers 1024]
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
    wid = snap.worker_id.tolist()
    where = {int(x): k for k, x in enumerate(ids.tolist())}
    rq_of = lambda x: int(rqs[where[x]])  # noqa: E731
    pr_of = lambda x: int(prio[where[x]])  # noqa: E731
    asg = [(tid, wid[w], v) for w, recs in enumerate(res.records) for (tid, v, k) in recs if k == abi.HQ_REC_ASSIGN]
    pf = [(tid, wid[w], 0) for w, recs in enumerate(res.records) for (tid, v, k) in recs if k == abi.HQ_REC_PREFILL]
    n_asg, n_pf, n_ready = len(asg), len(pf), t.ready_count()
    assert t.assigned_count() == n_asg and t.assigned_prefilled_count() == n_pf
    free0 = t.assigned_free_rows().copy()
    rng = np.random.default_rng(5)
    order = rng.permutation(n_asg)

    def state():
        return (t.assigned_count(), t.assigned_prefilled_count(), t.ready_count(), t.assigned_free_rows().tobytes())

    out = {"tasks": len(ids), "workers": W, "assigned": n_asg, "prefilled": n_pf, "ready": n_ready, "reps": args.reps, "host_waits_per_call": 2}
    batches = [(f"assigned_{k}", [asg[int(j)] for j in order[:k]], False) for k in (1, 16, 256, 4096) if k <= n_asg]
    if pf:
        batches.append(("prefilled_all", pf, True))
    for name, batch, prefilled in batches:
        b_id = np.asarray([b[0] for b in batch], np.uint64); b_w = np.asarray([b[1] for b in batch], np.uint32); b_v = np.asarray([b[2] for b in batch], np.uint8)
        back = sorted(b[0] for b in batch)
        s_id = np.asarray(back, np.uint64); s_pr = np.asarray([pr_of(x) for x in back], np.uint64); s_rq = np.asarray([rq_of(x) for x in back], np.uint32)
        lists = {}
        for (x, w, v) in batch:
            if (rq_of(x), v) not in lists.setdefault(w, []):
                lists[w].append((rq_of(x), v))
        workers = sorted(lists)
        entries = [(x, w, rq_of(x), v, pr_of(x)) for (x, w, v) in batch]
        seeds = [(x, w, rq_of(x), pr_of(x)) for (x, w, v) in batch]

        def restore():
            assert t.ready_remove(s_id) == len(batch)
            assert (t.assigned_track_prefilled(seeds) if prefilled else t.assigned_add(entries)) == len(batch)
            blocked = {w: t.cluster_blocked(w) for w in workers}
            for w in workers:
                t.cluster_set_blocked(w, [])
            assert t.assigned_count() == n_asg and t.assigned_prefilled_count() == n_pf and t.ready_count() == n_ready and (t.assigned_free_rows() == free0).all(), "not restored"
            return blocked

        t_new, t_old = [], []
        for rep in range(args.reps + 1):  # (the first round allocates the calls' staging: not timed)
            t0 = time.perf_counter(); got = t.reject_tasks(b_id, b_w, b_v); dt = time.perf_counter() - t0
            if rep:
                t_new.append(dt)
            assert got["accepted"] == len(batch) and [x[0] for x in got["requeued"]] == back
            after_new = state(); blocked_new = restore()
            t0 = time.perf_counter()
            done = t.assigned_unprefill(b_id) if prefilled else t.assigned_release(b_id)
            t.ready_add(s_id, s_pr, s_rq)
            for w in workers:
                t.cluster_set_blocked(w, lists[w])
            dt = time.perf_counter() - t0
            if rep:
                t_old.append(dt)
            assert done == len(batch) and state() == after_new
            assert restore() == blocked_new
        us = lambda x: [round(float(v) * 1e6, 1) for v in (np.median(x), np.min(x), np.max(x))]  # noqa: E731
        out[name] = {"n": len(batch), "workers": len(workers), "reject_call_us_p50_min_max": us(t_new), "parents_sequence_us_p50_min_max": us(t_old),
                     "ratio_new_over_parent": round(float(np.median(t_new) / np.median(t_old)), 3)}
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
