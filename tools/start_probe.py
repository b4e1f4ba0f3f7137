"""hqtick_start_tasks at c3p scale, with the protocol of tools/finish_probe.py: one MI355X, the c3p steady workload (1 M tasks, 1024 workers) in
the dependency graph, ledger and prefilled tracking on, one tick consumed.  Three batches: 1000 of the tick's assigned ids, all of them (shuffled), and all of the
tick's prefilled ids.  The state is restored (outside the timed part) before every timed call: started assigned entries are released and entered again, started
prefilled entries are released and the prefilled entries seeded again.  The prefilled batch has a counterpart at the parent commit, hqtick_assigned_start_prefilled
on the same ids, and both forms alternate; an _ASSIGNED batch has none (the parent has no call for it) and is reported as an absolute time.  Prints one JSON line:
per batch the p50 wall time of the whole handler with the min and max of the rounds.

    python tools/start_probe.py [--reps 5] [--tasks 1000000] [--workers 1024] [--only new|old]
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
    ap.add_argument("--only", choices=["new", "old"], default=None)
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
    asg = [(tid, wid[w], v) for w, recs in enumerate(res.records) for (tid, v, k) in recs if k == abi.HQ_REC_ASSIGN]
    pf = [(tid, wid[w]) for w, recs in enumerate(res.records) for (tid, v, k) in recs if k == abi.HQ_REC_PREFILL]
    assert t.assigned_count() == len(asg) and t.assigned_prefilled_count() == len(pf)
    entry = lambda tid, w, v: (tid, w, int(rqs[where[tid]]), v, int(prio[where[tid]]))  # noqa: E731
    pf_seed = [(tid, w, int(rqs[where[tid]]), int(prio[where[tid]])) for tid, w in pf]
    free0 = t.assigned_free_rows().copy()
    rng = np.random.default_rng(5)

    def restored(n_asg, n_pf):
        assert t.assigned_count() == n_asg and t.assigned_prefilled_count() == n_pf and (t.assigned_free_rows() == free0).all(), "the state was not restored"

    def restore_assigned(batch):
        assert t.assigned_release([b[0] for b in batch]) == len(batch)
        assert t.assigned_add([entry(*b) for b in batch]) == len(batch)
        restored(len(asg), len(pf))

    def restore_prefilled():
        assert t.assigned_release([p[0] for p in pf]) == len(pf)
        assert t.assigned_track_prefilled(pf_seed) == len(pf)
        if not (t.assigned_free_rows() == free0).all():  # a prefilled start may over-commit its worker (saturating free.remove): the release then gives back more than was taken
            t.cluster_update_workers(np.arange(W, dtype=np.uint32), free0)
        restored(len(asg), len(pf))

    out = {"tasks": len(ids), "workers": W, "assigned": len(asg), "prefilled": len(pf), "reps": args.reps}
    order = rng.permutation(len(asg))
    for name, batch in (("assigned_1000", [asg[int(k)] for k in order[:1000]]), ("assigned_all", [asg[int(k)] for k in order])):
        b_id = np.asarray([b[0] for b in batch], np.uint64); b_w = np.asarray([b[1] for b in batch], np.uint32); b_v = np.asarray([b[2] for b in batch], np.uint8)
        times = []
        for rep in range(args.reps + 1):  # (the first round allocates the call's staging: not timed)
            t0 = time.perf_counter(); got = t.start_tasks(b_id, b_w, b_v); dt = time.perf_counter() - t0
            if rep:
                times.append(dt)
            assert got["accepted"] == len(batch) and (got["kind"] == abi.HQ_START_ASSIGNED).all()
            restore_assigned(batch)
        out[name] = {"n": len(batch), "start_call_us_p50_min_max": [round(float(v) * 1e6, 1) for v in (np.median(times), np.min(times), np.max(times))]}
    if pf:
        p_id = np.asarray([p[0] for p in pf], np.uint64); p_w = np.asarray([p[1] for p in pf], np.uint32); p_v = np.zeros(len(pf), np.uint8)
        t_new, t_old = [], []
        for rep in range(args.reps + 1):
            if args.only != "old":
                t0 = time.perf_counter(); got = t.start_tasks(p_id, p_w, p_v); dt = time.perf_counter() - t0
                if rep:
                    t_new.append(dt)
                assert got["accepted"] == len(pf) and (got["kind"] == abi.HQ_START_PREFILLED).all()
                after_new = t.assigned_free_rows().copy()
                restore_prefilled()
            if args.only != "new":
                t0 = time.perf_counter(); done = t.assigned_start_prefilled(p_id, p_v); dt = time.perf_counter() - t0
                if rep:
                    t_old.append(dt)
                assert done == len(pf)
                if args.only is None:
                    assert (t.assigned_free_rows() == after_new).all()
                restore_prefilled()
        us = lambda x: [round(float(v) * 1e6, 1) for v in (np.median(x), np.min(x), np.max(x))] if x else None  # noqa: E731
        out["prefilled_all"] = {"n": len(pf), "start_call_us_p50_min_max": us(t_new), "parents_start_prefilled_us_p50_min_max": us(t_old)}
    print(json.dumps(out))
    t.close()


if __name__ == "__main__":
    main()
