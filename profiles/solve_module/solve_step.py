#!/usr/bin/env python
"""Once through every path of the placement's device side (hqsolve::Solver), for a kernel trace: a separable tick on k_block_solve, the same tick with a step budget
of 1, a coupled tick that takes the price sweeps, hqtick_query and hqtick_query_resident (each creates or reuses the sub-context), and a one-rank communicator's
hqtick_debug_exchange and hqtick_shard_allgather.
Run from the repository root (the library of that tree is the one loaded).

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/solve_module/solve_step.py
  python profiles/cluster_module/launch_sequence.py OUT
"""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from hyperqueue_amd import abi, workloads  # noqa: E402
from hyperqueue_amd.sharded import sink_layout  # noqa: E402
from hyperqueue_amd.tick import Tick  # noqa: E402

W, N = 48, 4000
UNIT = abi.HQ_FRACTIONS_PER_UNIT


def empty(snap: abi.Snapshot) -> abi.Snapshot:
    return dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))


def report(what: str, t: Tick, r: abi.Result):
    ks = t.kernel_stats()
    print(f"{what}: status {r.status}, {sum(len(x) for x in r.records)} records, {ks['n_classes_device']} classes on the device, {ks['n_classes_host']} on the host, "
          f"{ks['price_sweeps']} price sweeps")


os.environ["HQTICK_BLOCK_MIN_CLASSES"] = "1"  # (the knobs are read when a context is created)
steady = workloads.make_steady("c3", seed=0, n_tasks=N, n_workers=W)
cfg = abi.make_config(time_limit_s=20.0)

t = Tick(cfg)
report("separable tick", t, t.tick(steady))
t.close()

os.environ["HQTICK_BLOCK_BUDGET"] = "1"
t = Tick(cfg)
report("separable tick, budget 1", t, t.tick(steady))
t.close()
del os.environ["HQTICK_BLOCK_BUDGET"]

t = Tick(abi.make_config(time_limit_s=5.0))
report("coupled tick", t, t.tick(workloads.make("c3p", n_tasks=400_000, n_workers=256)))

ids = np.arange(4, dtype=np.uint32) + (1 << 20)
totals = np.zeros((4, steady.n_resources), np.uint64)
totals[0] = steady.worker_total[0]; totals[1, 0] = 1 * UNIT; totals[2, 0] = 16 * UNIT; totals[2, 2] = 8 * UNIT
loaded, opt = t.query(steady, ids, totals)
print(f"hqtick_query: loads {loaded.astype(int).tolist()}, optimal {opt}")
t.upload_ready(steady.task_id, steady.task_priority, steady.task_rq)
loaded, opt, rq_ready = t.query_resident(empty(steady), ids, totals)
print(f"hqtick_query_resident: loads {loaded.astype(int).tolist()}, optimal {opt}, {int(rq_ready.sum())} ready")
t.close()

t = Tick(cfg, measure=True)  # hqtick_debug_exchange: libhqtick_test.so
lib = t._lib
uid = (C.c_ubyte * 128)()
lib.hqtick_comm_unique_id.argtypes = [C.c_void_p]
lib.hqtick_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
lib.hqtick_debug_exchange.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
lib.hqtick_shard_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.hqtick_comm_destroy.argtypes = [C.c_void_p]
assert lib.hqtick_comm_unique_id(uid) == 0 and lib.hqtick_comm_init(t._ctx, uid, 0, 1) == 0
a = np.arange(4096, dtype=np.uint8); b = np.zeros(4096, np.uint8)
rc = lib.hqtick_debug_exchange(t._ctx, a.ctypes.data, b.ctypes.data, len(a))
print(f"hqtick_debug_exchange: {rc}, recv == send: {bool((a == b).all())}")
sink = torch.zeros(sink_layout(W, 1 << 13)[4], dtype=torch.uint8, device="cuda:0")
merged = torch.zeros_like(sink)
t.set_record_sink(sink, W)
r = t.tick(steady)
rc = lib.hqtick_shard_allgather(t._ctx, C.c_void_p(merged.data_ptr()), C.c_size_t(merged.numel()))
torch.cuda.synchronize()
print(f"hqtick_shard_allgather: {rc}, status {r.status}, gathered == sink: {bool((merged == sink).all())}, {int(sink[:4].cpu().numpy().view(np.uint32)[0])} records in the sink")
t.set_record_sink(None)
assert lib.hqtick_comm_destroy(t._ctx) == 0
t.close()
