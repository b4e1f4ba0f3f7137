#!/usr/bin/env python
"""Autoalloc query on c3p (1 M resident tasks, three priority levels, 1024 real workers): hqtick_query_resident against what a resident host
would do without it — flatten its mirror of the queues into id-sorted columns and call hqtick_query (which copies the 12 B/task priority and
request columns over PCIe).  Every repetition ends with hipDeviceSynchronize; p50 / p95 over --reps warmed repetitions, one JSON line.

    python tools/query_probe.py [--reps 101] [--warmup 5] [--tasks 1000000] [--out FILE]

The census kernel's own duration comes from a separate kernel-trace run of this probe (k_census in the trace's statistics)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402


def pct(xs, p):
    return float(np.percentile(np.asarray(xs), p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=101)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    snap = workloads.make("c3p", n_tasks=a.tasks)
    Q, R = len(snap.requests), snap.n_resources
    t = Tick(abi.make_config(time_limit_s=20.0))
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    empty = abi.Snapshot(**{**snap.__dict__, "task_id": np.zeros(0, np.uint64), "task_priority": np.zeros(0, np.uint64), "task_rq": np.zeros(0, np.uint32), "_keep": []})
    # the host mirror a resident host would otherwise keep: per request queue, its ids and priorities
    mirror = [(snap.task_id[snap.task_rq == q].copy(), snap.task_priority[snap.task_rq == q].copy()) for q in range(Q)]
    n_fake = 8
    ids = np.arange(1 << 20, (1 << 20) + n_fake, dtype=np.uint32)
    tot = np.full((n_fake, R), abi.HQ_AMOUNT_MAX, np.uint64)
    tot[:, 0] = 64 * abi.HQ_FRACTIONS_PER_UNIT   # partial query: 64 cpus, the other resources unbounded

    def resident():
        r = t.query_resident(empty, ids, tot)
        hip.hipDeviceSynchronize()
        return r

    def flatten_and_query():
        tid = np.concatenate([m[0] for m in mirror])
        pri = np.concatenate([m[1] for m in mirror])
        rq = np.concatenate([np.full(len(m[0]), q, np.uint32) for q, m in enumerate(mirror)])
        order = np.argsort(tid, kind="stable")
        full = abi.Snapshot(**{**snap.__dict__, "task_id": tid[order], "task_priority": pri[order], "task_rq": rq[order], "_keep": []})
        r = t.query(full, ids, tot)
        hip.hipDeviceSynchronize()
        return r

    a_l, a_o, rq_ready = resident()
    b_l, b_o = flatten_and_query()
    assert a_l.tobytes() == b_l.tobytes() and a_o == b_o, "the two paths disagree"
    assert (rq_ready == np.bincount(snap.task_rq.astype(np.int64), minlength=Q)).all()
    out = {"workload": "c3p", "n_tasks": int(a.tasks), "n_workers": len(snap.worker_id), "levels": int(len(np.unique(snap.task_priority))), "n_fake": n_fake,
           "reps": a.reps, "loaded": int(a_l.sum())}
    for name, fn in (("query_resident", resident), ("flatten_plus_query", flatten_and_query)):
        for _ in range(a.warmup):
            fn()
        us = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            us.append((time.perf_counter() - t0) * 1e6)
        out[name] = {"p50_us": round(pct(us, 50), 1), "p95_us": round(pct(us, 95), 1), "min_us": round(min(us), 1)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()
