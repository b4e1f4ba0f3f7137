"""Measurement of the resident attribute table of the wire encoder (hqwire_table_*, include/hqwire.h) at BASELINE C3 size on one MI355X.

    python tools/wire_table_probe.py [--steps 30] [--warmup 3] [--rows 1000000] [--out FILE]

One job.  STEP, on ~1 M resident rows with 8 configurations: an append of 188 416 fresh ids (1024 workers x 184 records), a remove of the 65 536 oldest
live ids, a view, and an encode of the 188 416-record tick over the fresh ids.  BASELINE, the same step done the only way possible without the table:
rebuild the host arrays (numpy) and upload the whole table, then encode.  The two alternate inside the job; every step's bytes are compared.
Host clock (perf_counter) around calls that end in a synchronisation, device events around view + encode; `*_device_us` of a table call is
hqwire_table_stats.last_kernel_us: events around everything the call enqueued (the batch's copy to the device, the kernels, the result block's copy back).  Then: encode on a view with 40 % dead rows
against the same table compacted; one forced compaction; one merge add.  Achieved bytes/s from the ALGORITHMIC bytes:
    append      37 B per row + its blob bytes, written once (the staging copy over PCIe is in the call's host time, not in this figure)
    compaction  (37 B + blob bytes) per live row, read once and written once
    remove      8 B per id read + one row probe (dependent loads: latency-bound, reported as ns per id)
as a share of the 8 TB/s HBM peak, here from the calls' device time (a lower bound on what the kernels reach).  Kernel times of the same job: run it once more under `rocprofv3 --kernel-trace --stats` (no counters, no other
tracing in that run).  Prints ONE JSON line; profiles/wire_table/README.md records a run."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
W, PER = 1024, 184
N_NEW, N_GONE = W * PER, 65536


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def summary(v):
    return {"p50": round(pct(v, 0.5), 1), "p10": round(pct(v, 0.1), 1), "p90": round(pct(v, 0.9), 1), "max": round(max(v), 1), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch  # first: its HIP runtime is the process's

    from hyperqueue_amd import wire

    lib, dev = wire.load(), torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(5)
    configs = [((3600, 0), b"body-of-class-%d" % i * 64) for i in range(8)]

    def columns(first, n):
        """n tasks with ids first.. : every fifth carries a 24-byte entry"""
        ids = (np.uint64(1 << 32) + np.arange(first, first + n, dtype=np.uint64))
        some = (np.arange(n) % 5 == 0).astype(np.uint8)
        lens = some.astype(np.uint64) * np.uint64(24)
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        return dict(task_id=ids, task_rq=rng.integers(0, 8, n).astype(np.uint32), task_instance=np.zeros(n, np.uint32),
                    task_priority=np.full(n, 0x8000000000000000, np.uint64), task_config=rng.integers(0, 8, n).astype(np.uint32), entry_some=some,
                    entry_off=off, entry_blob=rng.integers(0, 256, int(off[-1]), dtype=np.uint8))

    def records_for(ids):
        kind = np.tile((np.arange(PER) >= 120).astype(np.uint8), W)
        return wire.WireRecords(np.arange(1, W + 1, dtype=np.uint32), (np.arange(W + 1) * PER).astype(np.uint32), ids, np.where(kind == 1, 0, 0xFF).astype(np.uint8), kind,
                                np.zeros(W + 1, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.uint32), np.zeros(0, np.uint32))

    # ---- output buffers and the records' device copies, allocated once
    cap = 1 << 25
    zeros = lambda n: torch.zeros(max(8, int(n)), dtype=torch.uint8, device=dev)
    data, slot_off, status, header = zeros(cap), zeros(8 * (2 * W + 1)), zeros(W), zeros(16)
    scratch = zeros(int(lib.hqwire_scratch_bytes(N_NEW, W)) + 8)
    nfrag, frag_end = zeros(4 * W), zeros(8 * W * wire.HQWIRE_MAX_FRAGMENTS)
    oc = wire.OutputC(data.data_ptr(), cap, slot_off.data_ptr(), status.data_ptr(), header.data_ptr(), scratch.data_ptr(), scratch.numel(), nfrag.data_ptr(), frag_end.data_ptr(), 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def encode(tables_c, r):
        """-> (device us of [view +] encode, sha1 of the bytes); tables_c: a TablesC or a WireTable (then the view is taken inside the timed region)"""
        rt = wire._upload(torch, dev, r.arrays())
        torch.cuda.synchronize(dev)
        e0.record()
        tc = tables_c.view() if isinstance(tables_c, wire.WireTable) else tables_c
        rc = wire.RecordsC(r.n_workers, r.n_records, *[x.data_ptr() for x in rt[:7]], r.n_mn, *[x.data_ptr() for x in rt[7:]])
        if lib.hqwire_encode_device(C.byref(tc), C.byref(rc), C.byref(oc), C.c_void_p(stream)) != 0:
            raise RuntimeError("hqwire_encode_device failed")
        e1.record()
        torch.cuda.synchronize(dev)
        h = header.cpu().numpy().view(np.uint32)
        assert h[0] == 0 and int(status.max()) == 0, (h, int(status.max()))
        total = int(h[2]) | int(h[3]) << 32
        return 1000.0 * e0.elapsed_time(e1), hashlib.sha1(data[:total].cpu().numpy().tobytes()).hexdigest(), total

    # ---- the table and, for the baseline, the same tasks as host arrays
    table = wire.WireTable(initial_rows=1 << 23, initial_blob_bytes=1 << 28, stream=stream)
    table.add_configs(configs)
    host = columns(1, args.rows)
    t0 = time.perf_counter()
    table.add_tasks_arrays(**host)
    first_fill_ms = 1000 * (time.perf_counter() - t0)
    next_id = args.rows + 1  # (the baseline's host arrays hold live rows only)
    cfg_t = wire.WireTables.build({}, configs)

    def baseline_step(host, new, n_gone):
        """rebuild the live table's host arrays and upload all of them"""
        t0 = time.perf_counter()
        lens = np.diff(host["entry_off"])[n_gone:]
        b0 = int(host["entry_off"][n_gone])
        out = {}
        for k in ("task_id", "task_rq", "task_instance", "task_priority", "task_config", "entry_some"):
            out[k] = np.concatenate([host[k][n_gone:], new[k]])
        off = np.zeros(len(out["task_id"]) + 1, np.uint64)
        off[1:] = np.cumsum(np.concatenate([lens, np.diff(new["entry_off"])]))
        out["entry_off"] = off
        out["entry_blob"] = np.concatenate([host["entry_blob"][b0:], new["entry_blob"]])
        t1 = time.perf_counter()
        full = wire.WireTables(*[out[k] for k in ("task_id", "task_rq", "task_instance", "task_priority", "task_config", "entry_some", "entry_off", "entry_blob")],
                               *cfg_t.arrays()[8:])
        tt = wire._upload(torch, dev, full.arrays())
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        tc = wire.TablesC(full.n_tasks, *[x.data_ptr() for x in tt[:8]], full.n_configs, *[x.data_ptr() for x in tt[8:]])
        return out, tc, tt, 1e6 * (t1 - t0), 1e6 * (t2 - t1), sum(x.numel() for x in tt)

    m = {k: [] for k in ("append_us", "append_device_us", "remove_us", "remove_device_us", "view_encode_dev_us", "base_rebuild_us", "base_upload_us", "base_encode_dev_us")}
    upload_bytes = msg_bytes = 0
    for step in range(args.warmup + args.steps):
        new = columns(next_id, N_NEW)
        next_id += N_NEW
        n_gone = N_GONE
        gone = host["task_id"][:n_gone].copy()
        # -- the table: deltas
        t0 = time.perf_counter()
        table.add_tasks_arrays(**new)
        t1 = time.perf_counter()
        k_app = table.stats().last_kernel_us
        t2 = time.perf_counter()
        assert table.remove_tasks(gone) == n_gone
        t3 = time.perf_counter()
        k_rem = table.stats().last_kernel_us
        r = records_for(new["task_id"])
        dev_us, sha_t, msg_bytes = encode(table, r)
        # -- the baseline: rebuild + upload
        host, tc, keep, rebuild_us, upload_us, upload_bytes = baseline_step(host, new, n_gone)
        base_us, sha_b, _ = encode(tc, r)
        assert sha_t == sha_b, f"step {step}: the bytes of the two paths differ"
        del keep
        if step >= args.warmup:
            for k, v in (("append_us", 1e6 * (t1 - t0)), ("append_device_us", k_app), ("remove_us", 1e6 * (t3 - t2)), ("remove_device_us", k_rem), ("view_encode_dev_us", dev_us),
                         ("base_rebuild_us", rebuild_us), ("base_upload_us", upload_us), ("base_encode_dev_us", base_us)):
                m[k].append(v)
    st = table.stats()
    new_blob = int(np.diff(columns(0, N_NEW)["entry_off"]).sum())
    out = {"rows_start": args.rows, "steps": args.steps, "warmup": args.warmup, "n_new": N_NEW, "n_gone": N_GONE, "message_bytes": msg_bytes, "first_fill_ms": round(first_fill_ms, 1),
           "live_rows_end": int(st.live_rows), "physical_rows_end": int(st.physical_rows), "hbm_bytes": int(st.hbm_bytes), "baseline_upload_bytes": int(upload_bytes)}
    out.update({k: summary(v) for k, v in m.items()})
    app_bytes = 37 * N_NEW + new_blob
    out["append_GBps"] = round(app_bytes / (pct(m["append_device_us"], 0.5) * 1e-6) / 1e9, 1)
    out["append_share_of_hbm_peak"] = round(app_bytes / (pct(m["append_device_us"], 0.5) * 1e-6) / HBM_PEAK, 4)
    out["remove_ns_per_id"] = round(1000 * pct(m["remove_device_us"], 0.5) / N_GONE, 2)
    out["remove_GBps_of_8B_ids"] = round(8 * N_GONE / (pct(m["remove_device_us"], 0.5) * 1e-6) / 1e9, 2)

    # ---- one forced compaction of the table as the steps left it (the dead rows are the oldest ones, in front)
    s0 = table.stats()
    t0 = time.perf_counter()
    table.compact()
    out["compact_front_call_us"] = round(1e6 * (time.perf_counter() - t0), 1)
    out["compact_front_device_us"] = round(table.stats().last_kernel_us, 1)
    out["compact_front_rows"] = [int(s0.physical_rows), int(table.stats().physical_rows)]
    # ---- lookups on a view with 40 % dead rows against the same table compacted
    live = host["task_id"]
    dead_pick = np.sort(rng.choice(len(live) - N_NEW, int(0.4 * len(live)), replace=False))  # (the tick's tasks -- the newest N_NEW -- stay)
    assert table.remove_tasks(live[dead_pick]) == len(dead_pick)
    s1 = table.stats()
    r = records_for(live[-N_NEW:])
    with_dead = [encode(table, r) for _ in range(12)][2:]
    t0 = time.perf_counter()
    table.compact()
    compact_us = 1e6 * (time.perf_counter() - t0)
    s2 = table.stats()
    compacted = [encode(table, r) for _ in range(12)][2:]
    assert with_dead[0][1] == compacted[0][1]
    moved = 37 * int(s2.live_rows) + int(s2.blob_bytes)
    out["encode_dev_us_40pct_dead"] = summary([x[0] for x in with_dead])
    out["encode_dev_us_compacted"] = summary([x[0] for x in compacted])
    out["dead_fraction"] = round(1 - int(s1.live_rows) / int(s1.physical_rows), 3)
    out["compact_call_us"] = round(compact_us, 1)
    out["compact_device_us"] = round(s2.last_kernel_us, 1)
    out["compact_rows"] = int(s2.live_rows)
    out["compact_GBps_read_plus_written"] = round(2 * moved / (s2.last_kernel_us * 1e-6) / 1e9, 1)
    out["compact_share_of_hbm_peak"] = round(2 * moved / (s2.last_kernel_us * 1e-6) / HBM_PEAK, 4)
    # ---- one merge add: 1000 ids between resident ones (odd gaps do not exist in this id space, so: ids of removed rows come back)
    back = live[dead_pick][:: max(1, len(dead_pick) // 1000)][:1000]
    cols = columns(0, len(back))
    cols["task_id"] = back
    t0 = time.perf_counter()
    table.add_tasks_arrays(**cols)
    out["merge_call_us"] = round(1e6 * (time.perf_counter() - t0), 1)
    out["merge_device_us"] = round(table.stats().last_kernel_us, 1)
    out["merge_rows"] = int(table.stats().physical_rows)
    out["counters"] = table.counters()
    table.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
