"""hqtick_resident_check at c3p scale: what an audit of everything resident costs, and what leaving one behind every tick would cost.

    python tools/audit_profile.py [--tasks 1000000] [--workers 1024] [--waiting 250000] [--steps 12] [--calls 101] [--out profiles/audit/audit_profile.json]

The state: the c3p steady workload with the ledger and prefilled tracking on and EVERY task in the graph -- `tasks` ready ones and `waiting` more that wait for
three of them each -- after a few steps of the loop a reactor runs (release + finish what ran, new arrivals, a tick that consumes in
itself), so that the ledger holds a tick's worth of entries, the ready columns carry tombstones and the graph has free slots and stale edges.
  audit     hqtick_resident_check(HQ_CHECK_ALL | HQ_CHECK_STRICT) on that state: p50 of kernel_us (HIP events around the audit's device work) and of the call's
            wall clock (it ends in a stream synchronise) over `calls` calls after 10 warm-ups; the report must be clean.
  bytes     what each pass streams (the coalesced reads of its items, computed from the tables' sizes; the hash probes and the binary searches behind a live
            row are random 8-byte reads on top and are NOT counted) and the share of 8 TB/s those bytes over kernel_us come to.
  loop      the same step loop with and without one audit per tick, alternating, p50 of the step's wall clock.
One JSON line on stdout, and the same into --out.  No device: the run fails (there is no CPU path to time)."""
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

PARTS = abi.HQ_CHECK_ALL | abi.HQ_CHECK_STRICT
HBM_BYTES_PER_US = 8e6  # 8 TB/s


def _tick(t, snap):
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None; sc.prefilled_off = None; sc.prefilled_rq = None
    return t.tick_raw(sc, resident=True)


class Loop:
    """one context and the reactor's step on it"""

    def __init__(self, snap, waiting, seed):
        self.snap, self.W, self.R = snap, len(snap.worker_id), snap.n_resources
        self.t = t = Tick(abi.make_config(time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK | abi.HQTICK_FLAG_NO_KERNEL_TIMING))
        t.cluster_upload(snap)
        t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        t.assigned_enable([]); t.assigned_track_prefilled([])
        ids = np.asarray(snap.task_id, np.uint64)
        self._graph_add(ids, np.asarray(snap.task_priority, np.uint64), np.asarray(snap.task_rq, np.uint32), None)
        self.next_id = int(ids.max()) + 1
        if waiting:  # each waits for three ready tasks
            rng = np.random.default_rng(seed)
            w_ids = np.arange(self.next_id, self.next_id + waiting, dtype=np.uint64); self.next_id += waiting
            third = len(ids) // 3   # one producer out of each third of the ready tasks: three distinct ids
            dep = np.stack([rng.integers(0, third, waiting), third + rng.integers(0, third, waiting), 2 * third + rng.integers(0, third, waiting)], axis=1)
            self._graph_add(w_ids, np.zeros(waiting, np.uint64), (np.arange(waiting) % len(snap.requests)).astype(np.uint32), ids[dep])
        self.n_rq = len(snap.requests)
        self.prev = []

    def _graph_add(self, ids, prio, rq, deps):
        """hqtick_graph_add_tasks from arrays (deps: [n x k] producer ids, or None)"""
        import ctypes as C

        n = len(ids)
        off = np.arange(n + 1, dtype=np.uint32) * (0 if deps is None else deps.shape[1])
        flat = np.zeros(1, np.uint64) if deps is None else np.ascontiguousarray(deps.reshape(-1), np.uint64)
        f = self.t._lib.hqtick_graph_add_tasks
        f.argtypes = [C.c_void_p, C.c_uint64, abi.u64p, abi.u64p, abi.u32p, abi.u32p, abi.u64p]
        ids, prio, rq = np.ascontiguousarray(ids, np.uint64), np.ascontiguousarray(prio, np.uint64), np.ascontiguousarray(rq, np.uint32)
        return self.t._chk(f(self.t._ctx, n, ids.ctypes.data_as(abi.u64p), prio.ctypes.data_as(abi.u64p), rq.ctypes.data_as(abi.u32p), off.ctypes.data_as(abi.u32p),
                             flat.ctypes.data_as(abi.u64p)))

    def step(self, n_add, audit):
        t = self.t
        t0 = time.perf_counter()
        if self.prev:
            done = np.asarray(self.prev, np.uint64)
            t.assigned_release(done); t.graph_finish(done)
        add = np.arange(self.next_id, self.next_id + n_add, dtype=np.uint64); self.next_id += n_add
        self._graph_add(add, np.zeros(n_add, np.uint64), (np.arange(n_add) % self.n_rq).astype(np.uint32), None)
        r = _tick(t, self.snap)
        rep = t.resident_check(PARTS) if audit else None
        dt = time.perf_counter() - t0
        rec = abi.parse_result(r, self.W, self.R).records
        self.prev = [tid for recs in rec for (tid, v, k) in recs if k == abi.HQ_REC_ASSIGN]   # (prefilled tasks stay where they are: the ledger keeps them)
        if rep is not None:
            assert rep["failed"] == {} and rep["checked"] == PARTS, rep["failed"]
        return dt


def pass_bytes(t, W, R, n_ready_phys):
    """bytes each pass streams, from the sizes of the tables (hqtick.h: hqtick_graph_stats; the ledger's capacity is not exported: its entries x 4, the load the
    host keeps it under, rounded up to a power of two)"""
    g = t.graph_stats()
    n_slots, n_runs, n_edges = g["n_slots"], g["n_runs"], g["n_edges_pool"]
    entries = t.assigned_count() + t.assigned_prefilled_count() + t.assigned_mn_count()
    cap = 1 << max(10, int(np.ceil(np.log2(max(1, entries) * 4))))
    return {
        "ready_columns": n_ready_phys * (8 + 4),                      # id, request id
        "graph_slots_hash": n_slots * (4 + 8),                         # unfinished, id
        "graph_edges": n_slots * (4 + 4) + n_runs * 12 + n_edges * 8,  # unfinished, head; the run records; the edges
        "graph_counters": n_slots * (4 + 4 + 8),                       # unfinished, the census, id
        "ledger_buckets_estimate": cap * (8 + 1 + 4 + 4),              # key, variant, worker, request
        "ledger_rows": W * R * 16 + W * 10,                            # total, free; the multi-node columns (the count tables' widths are not exported)
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--workers", type=int, default=1024)
    ap.add_argument("--waiting", type=int, default=250_000)
    ap.add_argument("--add", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--calls", type=int, default=101)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    snap = workloads.make_steady("c3p", seed=3, n_tasks=args.tasks, n_workers=args.workers)
    W = len(snap.worker_id)
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], prefilled=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    a, b = Loop(snap, args.waiting, 1), Loop(snap, args.waiting, 1)
    ta, tb = [], []
    for k in range(args.steps):  # alternating: which loop goes first changes every step
        for loop, ts, audit in ((a, ta, True), (b, tb, False)) if k % 2 == 0 else ((b, tb, False), (a, ta, True)):
            ts.append(loop.step(args.add, audit))
    t = a.t
    for _ in range(10):
        t.resident_check(PARTS)
    ker, wall = [], []
    for _ in range(args.calls):
        t0 = time.perf_counter(); rep = t.resident_check(PARTS); wall.append((time.perf_counter() - t0) * 1e6); ker.append(rep["kernel_us"])
        assert rep["failed"] == {} and rep["checked"] == PARTS
    n_phys = args.tasks + args.steps * args.add  # an upper estimate of the physical rows (a compaction drops tombstones)
    pb = pass_bytes(t, W, snap.n_resources, n_phys)
    med = lambda x: round(float(np.median(x)), 1)  # noqa: E731
    skip = 2 if args.steps > 4 else 0
    out = {"tasks": args.tasks, "workers": W, "waiting": args.waiting, "added_per_step": args.add, "parts": PARTS,
           "ready_live": t.ready_count(), "graph": {k: v for k, v in t.graph_stats().items() if k != "last_kernel_us"},
           "ledger_entries": [t.assigned_count(), t.assigned_mn_count(), t.assigned_prefilled_count()],
           "audit_kernel_us_p50": med(ker), "audit_kernel_us_min": round(min(ker), 1), "audit_kernel_us_max": round(max(ker), 1), "audit_wall_us_p50": med(wall), "calls": args.calls,
           "pass_bytes_streamed": pb, "bytes_streamed": int(sum(pb.values())), "share_of_8TBps": round(sum(pb.values()) / med(ker) / HBM_BYTES_PER_US, 4),
           "step_wall_us_p50_with_audit": med(np.asarray(ta[skip:]) * 1e6), "step_wall_us_p50_without": med(np.asarray(tb[skip:]) * 1e6), "steps": args.steps}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")
    a.t.close(); b.t.close()


if __name__ == "__main__":
    main()
