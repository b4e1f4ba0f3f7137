"""Assignment ledger at c3p scale: a resident add -> tick -> release loop with the ledger (context A) against the same loop on today's
protocol (context B: the host keeps the free rows, sends the rows every start / finish touched, flattens the assigned CSR per tick).  Prints one JSON line:
per-step wall clock of both loops (B's host bookkeeping included), the release call for the previous step's tasks, and the ledger's tick-side apply.

    python tools/assigned_probe.py [--steps 20] [--tasks 1000000] [--workers 1024] [--records plain|compact|delta16|sink] [--mn K] [--prefill]

--records: the form in which context A's records leave the device (the ledger is fed from the mapping kernel's staging in HBM in every one of them; `sink`:
a device record sink, read back outside the timed part only to compare).  `ledger_host_bytes` is hqtick_assigned_last_host_bytes after the last tick.
--mn K: K two-node tasks run on the last 2 K workers throughout: every step releases them in the same batch as the single-node ids and seeds K new ones
on the same workers (hqtick_assigned_add_mn), so the release's row pass takes its multi-node branch; context B keeps those workers' SN bit clear with
hqtick_cluster_set_flags.  0 (the default) is the workload as it always was: no multi-node request, none of the new calls.
--prefill: context A tracks the prefilled tasks (hqtick_assigned_track_prefilled; its snapshots carry no prefilled CSR): a tick's PREFILL records enter the
ledger with its ASSIGN records, and every step starts the previous tick's prefilled tasks with hqtick_assigned_start_prefilled, behind the release of what
ran before; they are released one step later.  Context B does the same bookkeeping on the host (saturating free.remove, row deltas, assigned CSR).  Without
it the prefilled tasks of a tick are forgotten, as they always were in this loop.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

try:  # torch bundles its own HIP runtime: imported BEFORE libhqtick.so pulls in the system's, so that the process has one (--records sink hands it a tensor)
    import torch
except Exception:  # the other forms do not need it
    torch = None

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402


def _resident(t, snap, csr=None, prefilled_csr=True):
    sc = (csr or snap).to_c(resident_workers=True)
    if csr is None:
        sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
        if not prefilled_csr:
            sc.prefilled_off = None; sc.prefilled_rq = None
    return t.tick_raw(sc, resident=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--workers", type=int, default=1024)
    ap.add_argument("--add", type=int, default=188_000)
    ap.add_argument("--records", choices=["plain", "compact", "delta16", "sink"], default="plain")
    ap.add_argument("--mn", type=int, default=0)
    ap.add_argument("--prefill", action="store_true")
    args = ap.parse_args()
    snap = workloads.make_steady("c3p", seed=3, n_tasks=args.tasks, n_workers=args.workers)
    W, R = len(snap.worker_id), snap.n_resources
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    n_sn_rq = len(snap.requests)
    if args.mn:  # one two-node request class behind the others (no task of the ready set has it)
        assert 2 * args.mn < W
        snap = dataclasses.replace(snap, requests=list(snap.requests) + [[dict(entries=[(0, abi.HQ_ENTRY_AMOUNT, 10_000)], n_nodes=2, min_time_ns=0, weight=10_000)]], _keep=[])
    ent = [[[(int(r), int(k), int(a)) for (r, k, a) in v["entries"]] for v in rq] for rq in snap.requests]
    cfg = abi.make_config(time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK | abi.HQTICK_FLAG_NO_KERNEL_TIMING)
    form = {"plain": 0, "compact": abi.HQTICK_FLAG_COMPACT_RECORDS, "delta16": abi.HQTICK_FLAG_COMPACT_RECORDS | abi.HQTICK_FLAG_COMPACT_DELTA16, "sink": 0}[args.records]
    a, b = Tick(abi.make_config(time_limit_s=20.0, flags=cfg.flags | form)), Tick(cfg)
    for t in (a, b):
        t.cluster_upload(snap); t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    a.assigned_enable([])
    if args.prefill:
        a.assigned_track_prefilled([])
    mn_w = [[int(snap.worker_id[W - 2 * args.mn + 2 * i]), int(snap.worker_id[W - 2 * args.mn + 2 * i + 1])] for i in range(args.mn)]
    mn_ids, mn_next, tmn = [], 1 << 60, []
    if args.mn:
        b.cluster_set_flags([w for ws in mn_w for w in ws], [0] * (2 * args.mn))
    sink = None
    if args.records == "sink":
        from hyperqueue_amd.sharded import sink_layout

        sink = torch.zeros(sink_layout(W, 1 << 18)[4], dtype=torch.uint8, device="cuda:0")
        sink_cap = a.set_record_sink(sink, W)
    total = np.asarray(snap.worker_total, np.uint64).reshape(W, R)
    free = total.copy(); running = {}; rq_of = dict(zip(snap.task_id.tolist(), snap.task_rq.tolist()))
    next_id = int(snap.task_id.max()) + 1
    prev_a, prev_b = [], []
    pf_a, pf_b, run_pf_a, run_pf_b, tstart, n_pf = [], [], [], [], [], 0  # the last tick's prefilled tasks, and those started one step ago (still running)
    ta, tb, trel, ttick_a = [], [], [], []
    for step in range(args.steps):
        add = np.arange(next_id, next_id + args.add, dtype=np.uint64); next_id += args.add
        prio = np.zeros(len(add), np.uint64); rqs = (np.arange(len(add)) % n_sn_rq).astype(np.uint32)
        rq_of.update(zip(add.tolist(), rqs.tolist()))
        # A: release -> add -> tick
        t0 = time.perf_counter()
        if prev_a:
            t1 = time.perf_counter(); a.assigned_release(prev_a + run_pf_a + mn_ids); trel.append(time.perf_counter() - t1)
        if args.prefill and pf_a:
            ids = np.asarray(pf_a, np.uint64); zero = np.zeros(len(ids), np.uint8)
            t1 = time.perf_counter(); n_in = a.assigned_start_prefilled(ids, zero); tstart.append(time.perf_counter() - t1)
            assert n_in == len(pf_a) and a.assigned_prefilled_count() == 0
        run_pf_a = pf_a
        if args.mn:
            mn_ids = list(range(mn_next, mn_next + args.mn)); mn_next += args.mn
            t1 = time.perf_counter(); n_in = a.assigned_add_mn([(tid, n_sn_rq, 0, ws) for tid, ws in zip(mn_ids, mn_w)]); tmn.append(time.perf_counter() - t1)
            assert n_in == args.mn and a.assigned_mn_count() == args.mn
        a.ready_add(add, prio, rqs)
        t2 = time.perf_counter(); ra = _resident(a, snap, prefilled_csr=not args.prefill); ttick_a.append(time.perf_counter() - t2)
        ta.append(time.perf_counter() - t0)
        if sink is None:
            rec_a = abi.parse_result(ra, W, R).records
        else:  # the records are in the device tensor (layout: include/hqtick.h)
            h = sink.cpu().numpy()
            o_off, o_task, o_var, o_kind, _ = sink_layout(W, sink_cap)
            off = h[o_off:o_off + (W + 1) * 4].view(np.uint32).tolist(); n = off[W]
            col = list(zip(h[o_task:o_task + n * 8].view(np.uint64).tolist(), h[o_var:o_var + n].tolist(), h[o_kind:o_kind + n].tolist()))
            rec_a = [col[off[w]:off[w + 1]] for w in range(W)]
        prev_a = [tid for recs in rec_a for (tid, v, k) in recs if k == abi.HQ_REC_ASSIGN]
        if args.prefill:
            pf_a = [tid for recs in rec_a for (tid, v, k) in recs if k == abi.HQ_REC_PREFILL]
            assert a.assigned_prefilled_count() == len(pf_a)
            n_pf = len(pf_a)
        # B: the host's bookkeeping as today
        t0 = time.perf_counter()
        if prev_b:
            touched = set()
            for tid in prev_b + run_pf_b:
                w, q, v = running.pop(tid)
                for (res, kind, amount) in ent[q][v]:
                    free[w, res] = total[w, res] if kind == abi.HQ_ENTRY_ALL else free[w, res] + np.uint64(amount)
                touched.add(w)
            for tid, w in pf_b:  # task_from_prefilled_to_started: insert_sn_task with variant 0 (free.remove saturates)
                running[tid] = (w, rq_of[tid], 0)
                for (res, kind, amount) in ent[rq_of[tid]][0]:
                    free[w, res] = 0 if kind == abi.HQ_ENTRY_ALL else (free[w, res] - np.uint64(amount) if free[w, res] > amount else np.uint64(0))
                touched.add(w)
            run_pf_b = [tid for tid, _ in pf_b]
            idx = sorted(touched); b.cluster_update_workers(idx, free[idx])
        b.ready_add(add, prio, rqs)
        per_w = [[] for _ in range(W)]
        for tid, (w, q, v) in running.items():
            per_w[w].append((q, v))
        sb = dataclasses.replace(snap, assigned=per_w, worker_free=free.copy(), _keep=[])
        rb = abi.parse_result(_resident(b, snap, sb), W, R)
        nf = np.asarray(rb.new_free, np.uint64).reshape(W, R)
        changed = np.nonzero((nf != free).any(axis=1))[0].tolist(); free = nf.copy()
        if changed:
            b.cluster_update_workers(changed, free[changed])
        prev_b = []
        for w, recs in enumerate(rb.records):
            for (tid, v, k) in recs:
                if k == abi.HQ_REC_ASSIGN:
                    running[tid] = (w, rq_of[tid], v); prev_b.append(tid)
        pf_b = [(tid, w) for w, recs in enumerate(rb.records) for (tid, v, k) in recs if k == abi.HQ_REC_PREFILL] if args.prefill else []
        tb.append(time.perf_counter() - t0)
        assert rec_a == rb.records and a.assigned_count() == len(running)
    med = lambda x: round(float(np.median(x[2:] if len(x) > 4 else x)) * 1e6, 1)  # noqa: E731
    print(json.dumps({"steps": args.steps, "tasks": args.tasks, "workers": W, "added_per_step": args.add, "released_per_step": len(prev_a),
                      "step_us_ledger": med(ta), "step_us_row_deltas": med(tb), "release_call_us": med(trel), "tick_call_us_ledger": med(ttick_a),
                      "running": a.assigned_count(), "records": args.records, "ledger_host_bytes": a.assigned_last_host_bytes(),
                      **({"mn_tasks": args.mn, "add_mn_call_us": med(tmn)} if args.mn else {}),
                      **({"prefilled_per_step": n_pf, "start_prefilled_call_us": med(tstart) if tstart else None} if args.prefill else {})}))
    a.close(); b.close()


if __name__ == "__main__":
    main()
