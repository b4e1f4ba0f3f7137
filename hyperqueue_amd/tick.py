"""ctypes binding of libhqtick.so (include/hqtick.h).  The library is the product: there is no Python or CPU
implementation of the tick behind this module, and loading/creating a context fails loudly when the HIP library or
a gfx950 device is missing."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import abi

_LIB = None
_MLIB = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhqtick.so")
MEASURE_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhqtick_test.so")


class HqTickError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"hqtick error {code}: {msg}")
        self.code = code


def load(measure: bool = False):
    """the product library; measure=True: libhqtick_test.so — the same objects plus the measurement hooks of include/hqtick_debug.h (hqtick_time_kernel,
    hqtick_timeline, hqtick_block_profile_last) that the tools under tools/ use.  bench.py, the tests and smoke() run the product library."""
    global _LIB, _MLIB
    if measure:
        if _MLIB is None:
            _MLIB = _bind(C.CDLL(MEASURE_LIB_PATH))
        return _MLIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
        _LIB = _bind(C.CDLL(LIB_PATH))
    return _LIB


def _bind(lib):
    P = C.POINTER
    lib.hqtick_create.argtypes = [P(abi.Config), P(C.c_void_p)]
    lib.hqtick_destroy.argtypes = [C.c_void_p]
    lib.hqtick_run.argtypes = [C.c_void_p, P(abi.SnapshotC), P(abi.ResultC)]
    lib.hqtick_upload_ready.argtypes = [C.c_void_p, C.c_uint64, abi.u64p, abi.u64p, abi.u32p, C.c_int]
    lib.hqtick_run_resident.argtypes = [C.c_void_p, P(abi.SnapshotC), P(abi.ResultC)]
    lib.hqtick_query.argtypes = [C.c_void_p, P(abi.SnapshotC), P(abi.QueryWorkersC), P(abi.QueryResultC)]
    lib.hqtick_query_resident.argtypes = [C.c_void_p, P(abi.SnapshotC), P(abi.QueryWorkersC), P(abi.QueryResultC), abi.u64p]
    lib.hqtick_last_error.restype = C.c_char_p
    lib.hqtick_last_error.argtypes = [C.c_void_p]
    lib.hqtick_abi_version.restype = C.c_uint32
    lib.hqtick_build_arch.restype = C.c_char_p
    lib.hqtick_kernel_stats_last.argtypes = [C.c_void_p, P(abi.KernelStatsC)]
    return lib


class Tick:
    """One hqtick_ctx (one HIP device, one stream).  `tick(snapshot)` == run_scheduling_inner through the C ABI."""

    def __init__(self, config: Optional[abi.Config] = None, measure: bool = False):
        self.cfg = config or abi.make_config()
        extra = int(os.environ.get("HQTICK_TEST_FLAGS", "0") or 0)  # campaigns (tools/fuzz_more.py): the same scenarios through another emission form
        if extra:
            c = abi.Config.from_buffer_copy(self.cfg)
            c.flags |= extra
            self.cfg = c
        self._lib = load(measure)
        ctx = C.c_void_p()
        rc = self._lib.hqtick_create(C.byref(self.cfg), C.byref(ctx))
        if rc != 0:
            raise HqTickError(rc, "hqtick_create failed (no gfx950 device / HIP runtime?)")
        self._ctx = ctx
        self._add_packed = None

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.hqtick_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self) -> str:
        return self._lib.hqtick_last_error(self._ctx).decode()

    def tick_raw(self, sc: abi.SnapshotC, resident: bool = False) -> abi.ResultC:
        rc_ = abi.ResultC()
        fn = self._lib.hqtick_run_resident if resident else self._lib.hqtick_run
        rc = fn(self._ctx, C.byref(sc), C.byref(rc_))
        if rc < 0:
            raise HqTickError(rc, self._err())
        return rc_

    def tick(self, snap: abi.Snapshot, resident: bool = False, resident_workers: bool = False, resident_retracting: bool = False) -> abi.Result:
        """resident_workers: the snapshot travels without its worker side; the library completes it from its own worker set (hqtick_cluster_*, ABI 7).
        resident_retracting: the Retracting tasks of the queues come from the library's own table (hqtick_retracting_*, ABI 7)"""
        sc = snap.to_c(resident_workers=resident_workers)
        if resident_retracting:
            sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None; sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
        return abi.parse_result(self.tick_raw(sc, resident), len(snap.worker_id), snap.n_resources)

    def batches(self, snap: abi.Snapshot):
        return abi.parse_batches(self.tick_raw(snap.to_c()))

    def upload_ready(self, task_id: np.ndarray, task_priority: np.ndarray, task_rq: np.ndarray, sorted_: bool = True):
        a, b, c = (np.ascontiguousarray(task_id, np.uint64), np.ascontiguousarray(task_priority, np.uint64), np.ascontiguousarray(task_rq, np.uint32))
        rc = self._lib.hqtick_upload_ready(self._ctx, len(a), a.ctypes.data_as(abi.u64p), b.ctypes.data_as(abi.u64p), c.ctypes.data_as(abi.u32p), 1 if sorted_ else 0)
        if rc < 0:
            raise HqTickError(rc, self._err())

    # -- resident ready-set deltas (include/hqtick.h) -------------------------------------------------------
    def _chk(self, rc: int) -> int:
        if rc < 0:
            raise HqTickError(rc, self._err())
        return rc

    def ready_consume_last(self):
        self._lib.hqtick_ready_consume_last.argtypes = [C.c_void_p]
        self._chk(self._lib.hqtick_ready_consume_last(self._ctx))

    def ready_remove(self, task_id) -> int:
        a = np.ascontiguousarray(task_id, np.uint64)
        self._lib.hqtick_ready_remove.argtypes = [C.c_void_p, C.c_uint64, abi.u64p]
        return self._chk(self._lib.hqtick_ready_remove(self._ctx, len(a), a.ctypes.data_as(abi.u64p)))

    def ready_add(self, task_id, task_priority, task_rq):
        a, b, c = (np.ascontiguousarray(task_id, np.uint64), np.ascontiguousarray(task_priority, np.uint64), np.ascontiguousarray(task_rq, np.uint32))
        self._lib.hqtick_ready_add.argtypes = [C.c_void_p, C.c_uint64, abi.u64p, abi.u64p, abi.u32p]
        self._chk(self._lib.hqtick_ready_add(self._ctx, len(a), a.ctypes.data_as(abi.u64p), b.ctypes.data_as(abi.u64p), c.ctypes.data_as(abi.u32p)))

    def ready_add_stage(self, n: int):
        """(ids u64[n], priorities u64[n], rqs u32[n]) as numpy views of the library's pinned staging buffer: fill them, then ready_add_staged(n)"""
        pi, pp, pq = abi.u64p(), abi.u64p(), abi.u32p()
        self._lib.hqtick_ready_add_stage.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(abi.u64p), C.POINTER(abi.u64p), C.POINTER(abi.u32p)]
        self._chk(self._lib.hqtick_ready_add_stage(self._ctx, n, C.byref(pi), C.byref(pp), C.byref(pq)))
        if n == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        return (np.ctypeslib.as_array(pi, shape=(n,)), np.ctypeslib.as_array(pp, shape=(n,)), np.ctypeslib.as_array(pq, shape=(n,)))

    def ready_add_staged(self, n: int):
        self._lib.hqtick_ready_add_staged.argtypes = [C.c_void_p, C.c_uint64]
        self._chk(self._lib.hqtick_ready_add_staged(self._ctx, n))

    def ready_compact(self):
        self._lib.hqtick_ready_compact.argtypes = [C.c_void_p]
        self._chk(self._lib.hqtick_ready_compact(self._ctx))

    def ready_count(self) -> int:
        self._lib.hqtick_ready_count.restype = C.c_uint64
        self._lib.hqtick_ready_count.argtypes = [C.c_void_p]
        return int(self._lib.hqtick_ready_count(self._ctx))

    # -- cluster tables resident in HBM (include/hqtick.h, ABI 5) ------------------------------------------------------------
    def cluster_upload(self, snap):
        """worker rows + request tables of `snap` (abi.Snapshot or SnapshotC) -> HBM; later ticks read them there"""
        sc = snap.to_c() if hasattr(snap, "to_c") else snap
        self._lib.hqtick_cluster_upload.argtypes = [C.c_void_p, C.POINTER(abi.SnapshotC)]
        self._chk(self._lib.hqtick_cluster_upload(self._ctx, C.byref(sc)))
        self._asg_R = int(sc.n_resources)

    def cluster_update_workers(self, worker_index, free_rows, remaining_ns=None):
        """rows whose free resources (and optionally remaining lifetime) changed since the last call"""
        idx = np.ascontiguousarray(worker_index, np.uint32)
        rows = np.ascontiguousarray(free_rows, np.uint64).reshape(-1)
        rem = None if remaining_ns is None else np.ascontiguousarray(remaining_ns, np.int64)
        self._lib.hqtick_cluster_update_workers.argtypes = [C.c_void_p, C.c_uint32, abi.u32p, abi.u64p, C.POINTER(C.c_int64)]
        self._chk(self._lib.hqtick_cluster_update_workers(self._ctx, len(idx), idx.ctypes.data_as(abi.u32p), rows.ctypes.data_as(abi.u64p),
                                                          None if rem is None else rem.ctypes.data_as(C.POINTER(C.c_int64))))

    def cluster_add_workers(self, worker_id, total_rows, free_rows=None, remaining_ns=None, min_utilization=None, flags=None, group=None):
        """on_new_worker (ABI 7): ids ascending above every id present; they take the row indices W .. W + n - 1"""
        ids = np.ascontiguousarray(worker_id, np.uint32)
        tot = np.ascontiguousarray(total_rows, np.uint64).reshape(-1)
        fre = tot if free_rows is None else np.ascontiguousarray(free_rows, np.uint64).reshape(-1)
        opt = lambda a, dt, ct: (None, None) if a is None else (lambda v: (v, v.ctypes.data_as(C.POINTER(ct))))(np.ascontiguousarray(a, dt))
        rem, prem = opt(remaining_ns, np.int64, C.c_int64); mu, pmu = opt(min_utilization, np.float32, C.c_float); fl, pfl = opt(flags, np.uint8, C.c_uint8); gr, pgr = opt(group, np.uint32, C.c_uint32)
        self._lib.hqtick_cluster_add_workers.argtypes = [C.c_void_p, C.c_uint32, abi.u32p, abi.u64p, abi.u64p, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
        self._chk(self._lib.hqtick_cluster_add_workers(self._ctx, len(ids), ids.ctypes.data_as(abi.u32p), tot.ctypes.data_as(abi.u64p), fre.ctypes.data_as(abi.u64p), prem, pmu, pfl, pgr))

    def set_exchange(self, fn):
        """hqtick_set_exchange (ABI 8): fn(send_ptr, recv_ptr, bytes_per_rank) -> 0, an all-gather of host memory between the ranks of a sharded scheduler (the
        placement's price sweeps and class blocks are then split over the ranks); None removes it"""
        XFN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
        self._lib.hqtick_set_exchange.argtypes = [C.c_void_p, XFN, C.c_void_p]
        self._xfn = XFN((lambda _u, s, r, n: fn(s, r, n))) if fn is not None else XFN(0)  # kept alive with the Tick
        self._chk(self._lib.hqtick_set_exchange(self._ctx, self._xfn, None))

    def ready_add_packed(self, id_runs, prio_runs, task_rq, id_off=None):
        """hqtick_ready_add_packed (ABI 8): id_runs = [(first id, length)], prio_runs = [(priority, length)], task_rq u16 per task, id_off = None (consecutive ids inside a
        run) or u32 offsets from the run's first id — 2-6 bytes per task over PCIe instead of hqtick_ready_add's 20"""
        rq = np.ascontiguousarray(task_rq, np.uint16)
        ist = np.array([r[0] for r in id_runs], np.uint64); iln = np.array([r[1] for r in id_runs], np.uint32)
        pv = np.array([r[0] for r in prio_runs], np.uint64); pln = np.array([r[1] for r in prio_runs], np.uint32)
        off = None if id_off is None else np.ascontiguousarray(id_off, np.uint32)
        f = self._add_packed
        if f is None:  # (plain addresses: building five typed ctypes pointers per call costs more than the library spends preparing the launch)
            f = self._add_packed = self._lib.hqtick_ready_add_packed
            f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(f(self._ctx, len(rq), len(ist), ist.ctypes.data, iln.ctypes.data, off.ctypes.data if off is not None else None, len(pv), pv.ctypes.data, pln.ctypes.data, rq.ctypes.data))

    def cluster_remove_workers(self, worker_id):
        """on_remove_worker (ABI 7): by id; later rows move up.  Returns [(task, target worker id, variant)]: Retracting tasks of the removed workers that carried a
        redirect and are Assigned to its target from now on — the host sends their ComputeTasks messages (ABI 8, hqtick_cluster_last_reassigned)"""
        ids = np.ascontiguousarray(worker_id, np.uint32)
        self._lib.hqtick_cluster_remove_workers.argtypes = [C.c_void_p, C.c_uint32, abi.u32p]
        self._chk(self._lib.hqtick_cluster_remove_workers(self._ctx, len(ids), ids.ctypes.data_as(abi.u32p)))
        n = C.c_uint32(); pt, pw, pv = abi.u64p(), abi.u32p(), abi.u8p()
        self._lib.hqtick_cluster_last_reassigned.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
        self._chk(self._lib.hqtick_cluster_last_reassigned(self._ctx, C.byref(n), C.byref(pt), C.byref(pw), C.byref(pv)))
        k = n.value
        return list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pw, k, np.uint32).tolist(), abi._np(pv, k, np.uint8).tolist())) if k else []

    def cluster_set_blocked(self, worker_id: int, pairs):
        """Worker::blocked_requests of one worker := pairs of (rq, variant) (ABI 7)"""
        rq = np.ascontiguousarray([p[0] for p in pairs], np.uint32); v = np.ascontiguousarray([p[1] for p in pairs], np.uint8)
        self._lib.hqtick_cluster_set_blocked.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, abi.u32p, abi.u8p]
        self._chk(self._lib.hqtick_cluster_set_blocked(self._ctx, int(worker_id), len(pairs), rq.ctypes.data_as(abi.u32p) if len(pairs) else None, v.ctypes.data_as(abi.u8p) if len(pairs) else None))

    def cluster_workers(self) -> np.ndarray:
        n = C.c_uint32(); p = abi.u32p()
        self._lib.hqtick_cluster_workers.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u32p)]
        self._chk(self._lib.hqtick_cluster_workers(self._ctx, C.byref(n), C.byref(p)))
        return abi._np(p, n.value, np.uint32).copy() if n.value else np.zeros(0, np.uint32)

    def cluster_set_flags(self, worker_id, flags):
        """the HQ_WORKER_SN / HQ_WORKER_STOPPING bits of the listed resident workers, replaced (set_stop; set_mn_task / reset_mn_task without the ledger)"""
        ids = np.ascontiguousarray(worker_id, np.uint32); fl = np.ascontiguousarray(flags, np.uint8)
        assert len(ids) == len(fl)
        f = self._lib.hqtick_cluster_set_flags
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u32p, abi.u8p]
        self._chk(f(self._ctx, len(ids), ids.ctypes.data_as(abi.u32p), fl.ctypes.data_as(abi.u8p)))

    def cluster_worker_flags(self) -> np.ndarray:
        """the HQ_WORKER_* flags in row order"""
        n = C.c_uint32(); p = abi.u8p()
        f = self._lib.hqtick_cluster_worker_flags
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u8p)]
        self._chk(f(self._ctx, C.byref(n), C.byref(p)))
        return abi._np(p, n.value, np.uint8).copy() if n.value else np.zeros(0, np.uint8)

    def retracting_add(self, task_id, worker_id):
        """process_retracted outside a tick (ABI 7): tasks back in their queue as Retracting{worker id}"""
        t = np.ascontiguousarray(task_id, np.uint64); w = np.ascontiguousarray(worker_id, np.uint32)
        self._lib.hqtick_retracting_add.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p]
        self._chk(self._lib.hqtick_retracting_add(self._ctx, len(t), t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p)))

    def retract_response(self, worker_id: int, task_id):
        """on_retract_response (ABI 7) -> [(task, target worker id, variant)] of the tasks that are now Assigned to their redirect target"""
        t = np.ascontiguousarray(task_id, np.uint64)
        n = C.c_uint32(); pt, pw, pv = abi.u64p(), abi.u32p(), abi.u8p()
        self._lib.hqtick_retract_response.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, abi.u64p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
        self.last_retract_left = self._chk(self._lib.hqtick_retract_response(self._ctx, int(worker_id), len(t), t.ctypes.data_as(abi.u64p), C.byref(n), C.byref(pt), C.byref(pw), C.byref(pv)))  # tasks that left the table
        k = n.value
        return list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pw, k, np.uint32).tolist(), abi._np(pv, k, np.uint8).tolist())) if k else []

    def retracting_count(self) -> int:
        self._lib.hqtick_retracting_count.restype = C.c_uint32
        self._lib.hqtick_retracting_count.argtypes = [C.c_void_p]
        return int(self._lib.hqtick_retracting_count(self._ctx))

    # -- clock mode: termination times resident, a tick takes only the clock (include/hqtick.h) -----------------------------------
    def cluster_set_clock(self, now_ns: int):
        """the clock of the resident worker set; the first call turns the uploaded remaining lifetimes into termination times at now_ns"""
        f = self._lib.hqtick_cluster_set_clock
        f.argtypes = [C.c_void_p, C.c_int64]
        self._chk(f(self._ctx, int(now_ns)))

    def cluster_deadlines(self) -> np.ndarray:
        """the termination times in row order (HQ_NO_TIME_LIMIT: none); clock mode only"""
        n = C.c_uint32(); p = C.POINTER(C.c_int64)()
        f = self._lib.hqtick_cluster_deadlines
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_int64))]
        self._chk(f(self._ctx, C.byref(n), C.byref(p)))
        return abi._np(p, n.value, np.int64).copy() if n.value else np.zeros(0, np.int64)

    def cluster_last_row_groups(self) -> int:
        """groups of equal worker rows the host stages of the last tick found"""
        f = self._lib.hqtick_cluster_last_row_groups
        f.argtypes = [C.c_void_p]; f.restype = C.c_uint32
        return int(f(self._ctx))

    def cluster_drop(self):
        self._lib.hqtick_cluster_drop.argtypes = [C.c_void_p]
        self._chk(self._lib.hqtick_cluster_drop(self._ctx))

    # -- assignment ledger (include/hqtick.h, ABI 12) -------------------------------------------------------
    def _asg_cols(self, entries):
        """entries: [(task, worker id, rq, variant, priority)] -> five C columns"""
        t = np.ascontiguousarray([e[0] for e in entries], np.uint64); w = np.ascontiguousarray([e[1] for e in entries], np.uint32)
        q = np.ascontiguousarray([e[2] for e in entries], np.uint32); v = np.ascontiguousarray([e[3] for e in entries], np.uint8)
        p = np.ascontiguousarray([e[4] for e in entries], np.uint64)
        keep = (t, w, q, v, p)
        return keep, [t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p), q.ctypes.data_as(abi.u32p), v.ctypes.data_as(abi.u8p), p.ctypes.data_as(abi.u64p)]

    def assigned_enable(self, entries=()):
        """seed the ledger with [(task, worker id, rq, variant, priority)] (the free rows already count them)"""
        keep, cols = self._asg_cols(list(entries))
        f = self._lib.hqtick_assigned_enable
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u32p, abi.u8p, abi.u64p]
        self._chk(f(self._ctx, len(keep[0]), *cols))

    def assigned_disable(self):
        self._lib.hqtick_assigned_disable.argtypes = [C.c_void_p]
        self._chk(self._lib.hqtick_assigned_disable(self._ctx))

    def assigned_add(self, entries) -> int:
        """tasks that start outside a tick: [(task, worker id, rq, variant, priority)] -> number entered"""
        keep, cols = self._asg_cols(list(entries))
        f = self._lib.hqtick_assigned_add
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u32p, abi.u8p, abi.u64p]
        return self._chk(f(self._ctx, len(keep[0]), *cols))

    def assigned_release(self, task_id) -> int:
        """remove_sn_task for the ids, in batch order -> number released"""
        t = np.ascontiguousarray(task_id, np.uint64)
        f = self._lib.hqtick_assigned_release
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p]
        return self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p)))

    def assigned_add_mn(self, entries) -> int:
        """multi-node tasks seeded outside a tick: [(task, rq, priority, [worker ids, root first])] -> number entered"""
        entries = list(entries)
        t = np.ascontiguousarray([e[0] for e in entries], np.uint64); q = np.ascontiguousarray([e[1] for e in entries], np.uint32)
        p = np.ascontiguousarray([e[2] for e in entries], np.uint64)
        off = np.zeros(len(entries) + 1, np.uint32); off[1:] = np.cumsum([len(e[3]) for e in entries], dtype=np.uint64)
        w = np.ascontiguousarray([x for e in entries for x in e[3]], np.uint32)
        f = self._lib.hqtick_assigned_add_mn
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u64p, abi.u32p, abi.u32p]
        return self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), q.ctypes.data_as(abi.u32p), p.ctypes.data_as(abi.u64p), off.ctypes.data_as(abi.u32p),
                           w.ctypes.data_as(abi.u32p)))

    def assigned_mn_count(self) -> int:
        f = self._lib.hqtick_assigned_mn_count
        f.argtypes = [C.c_void_p]; f.restype = C.c_uint64
        return int(f(self._ctx))

    def assigned_mn_workers(self, task_id: int) -> list:
        """the multi-node task's current worker ids, root first ([]: not a multi-node task of the ledger)"""
        n = C.c_uint32(); p = abi.u32p()
        f = self._lib.hqtick_assigned_mn_workers
        f.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(abi.u32p)]
        self._chk(f(self._ctx, int(task_id), C.byref(n), C.byref(p)))
        return abi._np(p, n.value, np.uint32).tolist() if n.value else []

    def assigned_last_unknown(self) -> int:
        f = self._lib.hqtick_assigned_last_unknown
        f.argtypes = [C.c_void_p]; f.restype = C.c_uint64
        return int(f(self._ctx))

    def assigned_count(self) -> int:
        f = self._lib.hqtick_assigned_count
        f.argtypes = [C.c_void_p]; f.restype = C.c_uint64
        return int(f(self._ctx))

    def assigned_last_host_bytes(self) -> int:
        """bytes of record data the last placement's entry into the ledger copied from host memory to the device (0: the records stayed in HBM)"""
        f = self._lib.hqtick_assigned_last_host_bytes
        f.argtypes = [C.c_void_p]; f.restype = C.c_uint64
        return int(f(self._ctx))

    def set_record_sink(self, sink, n_workers: Optional[int] = None):
        """the tick's records go into `sink` (a contiguous device tensor of at least hqtick_sink_bytes(W, capacity) bytes, 16-byte aligned) instead of pinned
        host memory; None removes the sink.  n_workers given: returns how many records the tensor holds for that many workers.  The caller keeps the tensor alive."""
        f = self._lib.hqtick_set_record_sink
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        if sink is None:
            self._chk(f(self._ctx, None, 0))
            self._sink = None
            return 0
        nbytes = int(sink.numel() * sink.element_size())
        self._chk(f(self._ctx, C.c_void_p(sink.data_ptr()), C.c_size_t(nbytes)))
        self._sink = sink
        if n_workers is None:
            return 0
        g = self._lib.hqtick_sink_capacity_records
        g.argtypes = [C.c_uint32, C.c_size_t]; g.restype = C.c_uint32
        return int(g(int(n_workers), nbytes))

    def assigned_lookup(self, task_id):
        """-> (worker ids (HQ_NO_WORKER: not in the ledger), variants)"""
        t = np.ascontiguousarray(task_id, np.uint64)
        w = np.zeros(len(t), np.uint32); v = np.zeros(len(t), np.uint8)
        f = self._lib.hqtick_assigned_lookup
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u8p]
        self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p), v.ctypes.data_as(abi.u8p)))
        return w, v

    def assigned_free_rows(self) -> np.ndarray:
        n = C.c_uint32(); p = abi.u64p()
        f = self._lib.hqtick_assigned_free_rows
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p)]
        self._chk(f(self._ctx, C.byref(n), C.byref(p)))
        R = getattr(self, "_asg_R", 0)
        return abi._np(p, n.value * R, np.uint64).reshape(n.value, R).copy() if n.value and R else np.zeros((n.value, R), np.uint64)

    def cluster_last_requeued(self):
        """[(task, rq, priority)] the last cluster_remove_workers put back into the resident ready set (ABI 12)"""
        n = C.c_uint32(); pt, pq, pp = abi.u64p(), abi.u32p(), abi.u64p()
        f = self._lib.hqtick_cluster_last_requeued
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u64p)]
        self._chk(f(self._ctx, C.byref(n), C.byref(pt), C.byref(pq), C.byref(pp)))
        k = n.value
        return list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pq, k, np.uint32).tolist(), abi._np(pp, k, np.uint64).tolist())) if k else []

    # -- prefilled tasks in the ledger (SingleNodeTaskAssignment::prefilled_tasks; opt-in on top of assigned_enable) --------
    def assigned_track_prefilled(self, entries=()) -> int:
        """tracking on, seeded with [(task, worker id, rq, priority)] in state Prefilled -> number entered"""
        entries = list(entries)
        t = np.ascontiguousarray([e[0] for e in entries], np.uint64); w = np.ascontiguousarray([e[1] for e in entries], np.uint32)
        q = np.ascontiguousarray([e[2] for e in entries], np.uint32); p = np.ascontiguousarray([e[3] for e in entries], np.uint64)
        f = self._lib.hqtick_assigned_track_prefilled
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u32p, abi.u64p]
        return self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p), q.ctypes.data_as(abi.u32p), p.ctypes.data_as(abi.u64p)))

    def assigned_start_prefilled(self, started, variants=None) -> int:
        """task_from_prefilled_to_started for [(task, variant)] (or two columns: ids, variants) -> number started"""
        if variants is None:
            started = list(started)
            t = np.ascontiguousarray([e[0] for e in started], np.uint64); v = np.ascontiguousarray([e[1] for e in started], np.uint8)
        else:
            t = np.ascontiguousarray(started, np.uint64); v = np.ascontiguousarray(variants, np.uint8)
            assert len(t) == len(v)
        f = self._lib.hqtick_assigned_start_prefilled
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u8p]
        return self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), v.ctypes.data_as(abi.u8p)))

    def assigned_unprefill(self, task_id) -> int:
        """remove_prefill_task for the ids (prefill disposal, cancel, reject outside a tick) -> number removed"""
        t = np.ascontiguousarray(task_id, np.uint64)
        f = self._lib.hqtick_assigned_unprefill
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p]
        return self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p)))

    def assigned_prefilled_count(self) -> int:
        f = self._lib.hqtick_assigned_prefilled_count
        f.argtypes = [C.c_void_p]; f.restype = C.c_uint64
        return int(f(self._ctx))

    def cluster_last_requeued_prefilled(self) -> list:
        """the ids among cluster_last_requeued() that were prefilled on a lost worker, ascending"""
        n = C.c_uint32(); pt = abi.u64p()
        f = self._lib.hqtick_cluster_last_requeued_prefilled
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p)]
        self._chk(f(self._ctx, C.byref(n), C.byref(pt)))
        return abi._np(pt, n.value, np.uint64).tolist() if n.value else []

    # -- on_cancel_tasks in one call (include/hqtick.h) ------------------------------------------------------
    def cancel_tasks(self, task_id, as_csr: bool = False) -> dict:
        """hqtick_cancel_tasks for the ids, in this order -> {"messages": {worker id: [ids]} (the CancelTasks lists, workers ascending, ids in batch order; as_csr: the
        three arrays (worker ids, offsets, ids) as views of the context's pinned memory, valid until the next call),
        "n_ids": ids in the messages, "route_worker" / "route_kind": per batch position the worker id (HQ_NO_WORKER: none) and the HQ_CANCEL_* kind,
        "ready_removed": tasks that left the resident ready set, "closure": hqtick_graph_last_ids (what left the graph), "graph_unknown"}"""
        t = np.ascontiguousarray(task_id, np.uint64)
        f = self._lib.hqtick_cancel_tasks
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p]
        n_ids = self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p)))
        nw = C.c_uint32(); pw, po, pt = abi.u32p(), abi.u32p(), abi.u64p()
        g = self._lib.hqtick_cancel_last_messages
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u32p), C.POINTER(abi.u32p), C.POINTER(abi.u64p)]
        self._chk(g(self._ctx, C.byref(nw), C.byref(pw), C.byref(po), C.byref(pt)))
        messages = {}
        if nw.value:
            wid = abi._np(pw, nw.value, np.uint32); off = abi._np(po, nw.value + 1, np.uint32); ids = abi._np(pt, int(off[nw.value]), np.uint64)
            messages = (wid, off, ids) if as_csr else {int(wid[k]): ids[off[k]:off[k + 1]].tolist() for k in range(nw.value)}
        elif as_csr:
            messages = (np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(0, np.uint64))
        nr = C.c_uint32(); rw, rk = abi.u32p(), abi.u8p()
        h = self._lib.hqtick_cancel_last_routes
        h.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
        self._chk(h(self._ctx, C.byref(nr), C.byref(rw), C.byref(rk)))
        k = nr.value
        r = self._lib.hqtick_cancel_last_ready_removed
        r.argtypes = [C.c_void_p]; r.restype = C.c_uint64
        self._lib.hqtick_graph_last_unknown.restype = C.c_uint64
        self._lib.hqtick_graph_last_unknown.argtypes = [C.c_void_p]
        return {"messages": messages, "n_ids": int(n_ids),
                "route_worker": abi._np(rw, k, np.uint32).copy() if k else np.zeros(0, np.uint32), "route_kind": abi._np(rk, k, np.uint8).copy() if k else np.zeros(0, np.uint8),
                "ready_removed": int(r(self._ctx)), "closure": self._graph_last_ids(), "graph_unknown": int(self._lib.hqtick_graph_last_unknown(self._ctx))}

    # -- task_finished in one call (include/hqtick.h) --------------------------------------------------------
    def finish_tasks(self, task_id, worker_id) -> dict:
        """hqtick_finish_tasks for the (id, reporting worker) pairs, in this order -> {"accepted": positions accepted (need_scheduling), "kind": per batch position
        the HQ_FINISH_* kind, "released": hqtick_graph_last_ids (the consumers that joined the ready set), "graph_unknown": hqtick_graph_last_unknown}"""
        t = np.ascontiguousarray(task_id, np.uint64); w = np.ascontiguousarray(worker_id, np.uint32)
        assert len(t) == len(w)
        f = self._lib.hqtick_finish_tasks
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p]
        accepted = self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p)))
        n = C.c_uint32(); pk = abi.u8p()
        g = self._lib.hqtick_finish_last_routes
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u8p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pk)))
        self._lib.hqtick_graph_last_unknown.restype = C.c_uint64
        self._lib.hqtick_graph_last_unknown.argtypes = [C.c_void_p]
        return {"accepted": int(accepted), "kind": abi._np(pk, n.value, np.uint8).copy() if n.value else np.zeros(0, np.uint8),
                "released": self._graph_last_ids(), "graph_unknown": int(self._lib.hqtick_graph_last_unknown(self._ctx))}

    # -- task_failed in one call (include/hqtick.h) ----------------------------------------------------------
    def fail_tasks(self, task_id, worker_id) -> dict:
        """hqtick_fail_tasks for the (id, reporting worker or HQ_NO_WORKER) pairs, in this order -> {"accepted": positions accepted, "kind": per batch position the
        HQ_FAIL_* kind, "consumer_off" [n + 1] / "consumer_id": per position the tasks it removed beyond its own (ascending), "removed": hqtick_graph_last_ids
        (the accepted ids and all lists), "graph_unknown": hqtick_graph_last_unknown}"""
        t = np.ascontiguousarray(task_id, np.uint64); w = np.ascontiguousarray(worker_id, np.uint32)
        assert len(t) == len(w)
        f = self._lib.hqtick_fail_tasks
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p]
        accepted = self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p)))
        return {"accepted": int(accepted), **self.fail_last()}

    def fail_last(self) -> dict:
        """hqtick_fail_last_routes / hqtick_fail_last_consumers and the graph's last ids as numpy copies (also after a call that returned an error)"""
        n = C.c_uint32(); pk = abi.u8p()
        g = self._lib.hqtick_fail_last_routes
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u8p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pk)))
        m = C.c_uint32(); po = abi.u32p(); pi = abi.u64p()
        h = self._lib.hqtick_fail_last_consumers
        h.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u32p), C.POINTER(abi.u64p)]
        self._chk(h(self._ctx, C.byref(m), C.byref(po), C.byref(pi)))
        off = abi._np(po, m.value + 1, np.uint32).copy()
        total = int(off[-1])
        self._lib.hqtick_graph_last_unknown.restype = C.c_uint64
        self._lib.hqtick_graph_last_unknown.argtypes = [C.c_void_p]
        return {"kind": abi._np(pk, n.value, np.uint8).copy() if n.value else np.zeros(0, np.uint8), "consumer_off": off,
                "consumer_id": abi._np(pi, total, np.uint64).copy() if total else np.zeros(0, np.uint64),
                "removed": self._graph_last_ids(), "graph_unknown": int(self._lib.hqtick_graph_last_unknown(self._ctx))}

    def retracting_started(self, started) -> int:
        """hqtick_retracting_started for [(task, worker id it runs on, rq, variant, priority)]: task_running of Retracting tasks -> number started"""
        started = list(started)
        t = np.ascontiguousarray([e[0] for e in started], np.uint64); w = np.ascontiguousarray([e[1] for e in started], np.uint32)
        q = np.ascontiguousarray([e[2] for e in started], np.uint32); v = np.ascontiguousarray([e[3] for e in started], np.uint8)
        p = np.ascontiguousarray([e[4] for e in started], np.uint64)
        f = self._lib.hqtick_retracting_started
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u32p, abi.u8p, abi.u64p]
        return self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p), q.ctypes.data_as(abi.u32p), v.ctypes.data_as(abi.u8p),
                           p.ctypes.data_as(abi.u64p)))

    # -- task_running in one call (include/hqtick.h) ---------------------------------------------------------
    def start_tasks(self, task_id, worker_id, variant, rq=None, priority=None) -> dict:
        """hqtick_start_tasks for the (id, reporting worker, variant) triples, in this order; rq / priority: the tasks' own (None: NULL, allowed while the Retracting
        table is empty) -> {"accepted": positions accepted, "kind": per batch position the HQ_START_* kind}"""
        t = np.ascontiguousarray(task_id, np.uint64); w = np.ascontiguousarray(worker_id, np.uint32); v = np.ascontiguousarray(variant, np.uint8)
        assert len(t) == len(w) == len(v)
        q = None if rq is None else np.ascontiguousarray(rq, np.uint32); p = None if priority is None else np.ascontiguousarray(priority, np.uint64)
        assert (q is None or len(q) == len(t)) and (p is None or len(p) == len(t))
        f = self._lib.hqtick_start_tasks
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u8p, abi.u32p, abi.u64p]
        accepted = self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p), v.ctypes.data_as(abi.u8p),
                               None if q is None else q.ctypes.data_as(abi.u32p), None if p is None else p.ctypes.data_as(abi.u64p)))
        return {"accepted": int(accepted), "kind": self.start_last_routes()}

    def start_last_routes(self) -> np.ndarray:
        """hqtick_start_last_routes as a numpy copy (also after a call that returned an error)"""
        n = C.c_uint32(); pk = abi.u8p()
        g = self._lib.hqtick_start_last_routes
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u8p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pk)))
        return abi._np(pk, n.value, np.uint8).copy() if n.value else np.zeros(0, np.uint8)

    def assigned_running(self, task_id) -> np.ndarray:
        """hqtick_assigned_running: per id the running byte of its ledger entry (0 / 1; 0xFF: no entry)"""
        t = np.ascontiguousarray(task_id, np.uint64)
        r = np.zeros(len(t), np.uint8)
        f = self._lib.hqtick_assigned_running
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u8p]
        self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), r.ctypes.data_as(abi.u8p)))
        return r

    def cluster_last_requeued_running(self) -> list:
        """the ids among cluster_last_requeued() that were running on a lost worker (on_remove_worker's running_tasks), ascending"""
        n = C.c_uint32(); pt = abi.u64p()
        f = self._lib.hqtick_cluster_last_requeued_running
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p)]
        self._chk(f(self._ctx, C.byref(n), C.byref(pt)))
        return abi._np(pt, n.value, np.uint64).tolist() if n.value else []

    # -- task_reject / request_enabled in one call (include/hqtick.h) ------------------------------------------
    def reject_tasks(self, task_id, worker_id, variant, rq=None) -> dict:
        """hqtick_reject_tasks for the (id, reporting worker, rejected variant) triples, in this order; a variant of None or 0xFF names none; rq: the tasks' own
        requests (None: NULL, allowed while the Retracting table is empty) -> {"accepted": positions accepted, "kind": per batch position the HQ_REJECT_* kind,
        "requeued": [(task, rq, priority)] that went back into the ready set, ids ascending, "reassigned": [(task, redirect target, variant)]}"""
        t = np.ascontiguousarray(task_id, np.uint64); w = np.ascontiguousarray(worker_id, np.uint32)
        v = np.ascontiguousarray([abi.HQ_VARIANT_NONE if x is None else x for x in variant], np.uint8)
        assert len(t) == len(w) == len(v)
        q = None if rq is None else np.ascontiguousarray(rq, np.uint32)
        assert q is None or len(q) == len(t)
        f = self._lib.hqtick_reject_tasks
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u8p, abi.u32p]
        accepted = self._chk(f(self._ctx, len(t), t.ctypes.data_as(abi.u64p), w.ctypes.data_as(abi.u32p), v.ctypes.data_as(abi.u8p), None if q is None else q.ctypes.data_as(abi.u32p)))
        return dict(accepted=int(accepted), **self.reject_last())

    def reject_last(self) -> dict:
        """hqtick_reject_last_routes / _last_requeued / _last_reassigned as copies (also after a call that returned an error)"""
        n = C.c_uint32(); pk = abi.u8p()
        g = self._lib.hqtick_reject_last_routes
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u8p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pk)))
        kind = abi._np(pk, n.value, np.uint8).copy() if n.value else np.zeros(0, np.uint8)
        pt, pq, pp = abi.u64p(), abi.u32p(), abi.u64p()
        g = self._lib.hqtick_reject_last_requeued
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u64p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pt), C.byref(pq), C.byref(pp)))
        k = n.value
        requeued = list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pq, k, np.uint32).tolist(), abi._np(pp, k, np.uint64).tolist())) if k else []
        pw, pv = abi.u32p(), abi.u8p()
        g = self._lib.hqtick_reject_last_reassigned
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pt), C.byref(pw), C.byref(pv)))
        k = n.value
        reassigned = list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pw, k, np.uint32).tolist(), abi._np(pv, k, np.uint8).tolist())) if k else []
        return dict(kind=kind, requeued=requeued, reassigned=reassigned)

    # -- on_remove_worker in one call (include/hqtick.h) ----------------------------------------------------------
    def lose_workers(self, worker_ids) -> dict:
        """hqtick_lose_workers for the lost workers, in this order -> {"n_requeued": tasks that went back into the ready set, "per_worker": per lost worker (the
        caller's order) its [(task, rq, priority, HQ_LOSE_* kind)], ids ascending, "requeued": [(task, rq, priority)] of all of them, ids ascending, "reassigned":
        [(task, redirect target, variant)], "mn_left": [(task, lost worker, root worker)]}"""
        ids = np.ascontiguousarray(worker_ids, np.uint32)
        f = self._lib.hqtick_lose_workers
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u32p]
        n = self._chk(f(self._ctx, len(ids), ids.ctypes.data_as(abi.u32p) if len(ids) else None))
        return dict(n_requeued=int(n), **self.lose_last())

    def lose_last(self) -> dict:
        """hqtick_lose_last_tasks / _last_requeued / _last_reassigned / _last_mn_left as copies (also after a call that returned an error)"""
        n = C.c_uint32(); po, pt, pq, pp, pk = abi.u32p(), abi.u64p(), abi.u32p(), abi.u64p(), abi.u8p()
        g = self._lib.hqtick_lose_last_tasks
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u32p), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u64p), C.POINTER(abi.u8p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(po), C.byref(pt), C.byref(pq), C.byref(pp), C.byref(pk)))
        per_worker = []
        if n.value:
            off = abi._np(po, n.value + 1, np.uint32).tolist()
            k = off[-1]
            rows = list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pq, k, np.uint32).tolist(), abi._np(pp, k, np.uint64).tolist(), abi._np(pk, k, np.uint8).tolist())) if k else []
            per_worker = [rows[off[i]:off[i + 1]] for i in range(n.value)]
        g = self._lib.hqtick_lose_last_requeued
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u64p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pt), C.byref(pq), C.byref(pp)))
        k = n.value
        requeued = list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pq, k, np.uint32).tolist(), abi._np(pp, k, np.uint64).tolist())) if k else []
        pw, pv = abi.u32p(), abi.u8p()
        g = self._lib.hqtick_lose_last_reassigned
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pt), C.byref(pw), C.byref(pv)))
        k = n.value
        reassigned = list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pw, k, np.uint32).tolist(), abi._np(pv, k, np.uint8).tolist())) if k else []
        pr = abi.u32p()
        g = self._lib.hqtick_lose_last_mn_left
        g.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u32p)]
        self._chk(g(self._ctx, C.byref(n), C.byref(pt), C.byref(pw), C.byref(pr)))
        k = n.value
        mn_left = list(zip(abi._np(pt, k, np.uint64).tolist(), abi._np(pw, k, np.uint32).tolist(), abi._np(pr, k, np.uint32).tolist())) if k else []
        return dict(per_worker=per_worker, requeued=requeued, reassigned=reassigned, mn_left=mn_left)

    def cluster_enable_request(self, worker_id: int, rq: int, variant: int) -> int:
        """hqtick_cluster_enable_request (request_enabled): the pair leaves the worker's blocked set -> 1 if it was there, else 0"""
        f = self._lib.hqtick_cluster_enable_request
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint8]
        return self._chk(f(self._ctx, int(worker_id), int(rq), int(variant)))

    def cluster_blocked(self, worker_id: int) -> list:
        """hqtick_cluster_blocked: [(rq, variant)] of one worker's blocked set, in the order the pairs were added"""
        n = C.c_uint32(); pq, pv = abi.u32p(), abi.u8p()
        f = self._lib.hqtick_cluster_blocked
        f.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
        self._chk(f(self._ctx, int(worker_id), C.byref(n), C.byref(pq), C.byref(pv)))
        return list(zip(abi._np(pq, n.value, np.uint32).tolist(), abi._np(pv, n.value, np.uint8).tolist())) if n.value else []

    # -- device-resident dependency graph (include/hqtick.h) --------------------------------------------------
    def _graph_last_ids(self) -> np.ndarray:
        n = C.c_uint64()
        self._lib.hqtick_graph_last_ids.restype = abi.u64p
        self._lib.hqtick_graph_last_ids.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        p = self._lib.hqtick_graph_last_ids(self._ctx, C.byref(n))
        return abi._np(p, n.value, np.uint64).copy() if n.value else np.zeros(0, np.uint64)

    def graph_add_tasks(self, task_id, task_priority, task_rq, deps) -> np.ndarray:
        """on_new_tasks (reactor.rs:188-220).  `deps` = one list of task ids per task, or a (dep_off, dep_task_id) CSR pair.
        Returns the ids that are ready now (ascending); they are already merged into the resident ready set."""
        a, b, c = (np.ascontiguousarray(task_id, np.uint64), np.ascontiguousarray(task_priority, np.uint64), np.ascontiguousarray(task_rq, np.uint32))
        if isinstance(deps, tuple):
            off, dep = np.ascontiguousarray(deps[0], np.uint32), np.ascontiguousarray(deps[1], np.uint64)
        else:
            off = np.zeros(len(a) + 1, np.uint32)
            off[1:] = np.cumsum([len(d) for d in deps])
            dep = np.ascontiguousarray([x for d in deps for x in d], np.uint64)
        self._lib.hqtick_graph_add_tasks.argtypes = [C.c_void_p, C.c_uint64, abi.u64p, abi.u64p, abi.u32p, abi.u32p, abi.u64p]
        self._chk(self._lib.hqtick_graph_add_tasks(self._ctx, len(a), a.ctypes.data_as(abi.u64p), b.ctypes.data_as(abi.u64p), c.ctypes.data_as(abi.u32p),
                                                   off.ctypes.data_as(abi.u32p), dep.ctypes.data_as(abi.u64p)))
        return self._graph_last_ids()

    def graph_finish(self, task_id) -> tuple[np.ndarray, int]:
        """task_finished (reactor.rs:510-590) for a batch.  Returns (released ids ascending, number of unknown ids)."""
        a = np.ascontiguousarray(task_id, np.uint64)
        self._lib.hqtick_graph_finish.argtypes = [C.c_void_p, C.c_uint64, abi.u64p]
        self._chk(self._lib.hqtick_graph_finish(self._ctx, len(a), a.ctypes.data_as(abi.u64p)))
        self._lib.hqtick_graph_last_unknown.restype = C.c_uint64
        self._lib.hqtick_graph_last_unknown.argtypes = [C.c_void_p]
        return self._graph_last_ids(), int(self._lib.hqtick_graph_last_unknown(self._ctx))

    def graph_remove(self, task_id, recursive: bool = False) -> np.ndarray:
        """Core::remove_task (core.rs:222-240), with the transitive consumers if `recursive` (task.rs:235-250).  Returns the removed ids."""
        a = np.ascontiguousarray(task_id, np.uint64)
        self._lib.hqtick_graph_remove.argtypes = [C.c_void_p, C.c_uint64, abi.u64p, C.c_int]
        self._chk(self._lib.hqtick_graph_remove(self._ctx, len(a), a.ctypes.data_as(abi.u64p), 1 if recursive else 0))
        return self._graph_last_ids()

    def graph_blevel(self, update_ready: bool = False) -> dict:
        """EXTENSION (include/hqtick.h: hqtick_graph_blevel; no reference counterpart, parity unpinned): b-levels into the low 32 bits of the graph's priorities."""
        mx, upd = C.c_uint32(0), C.c_uint32(0)
        self._lib.hqtick_graph_blevel.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        rc = self._lib.hqtick_graph_blevel(self._ctx, 1 if update_ready else 0, C.byref(mx), C.byref(upd))
        if rc < 0:
            self._chk(rc)
        return {"sweeps": int(rc), "max_level": int(mx.value), "ready_updated": int(upd.value)}

    def graph_priorities(self, task_id) -> np.ndarray:
        a = np.ascontiguousarray(task_id, np.uint64)
        out = np.zeros(len(a), np.uint64)
        self._lib.hqtick_graph_priorities.argtypes = [C.c_void_p, C.c_uint64, abi.u64p, abi.u64p]
        self._chk(self._lib.hqtick_graph_priorities(self._ctx, len(a), a.ctypes.data_as(abi.u64p), out.ctypes.data_as(abi.u64p)))
        return out

    def graph_unfinished(self, task_id) -> np.ndarray:
        a = np.ascontiguousarray(task_id, np.uint64)
        out = np.zeros(len(a), np.uint32)
        self._lib.hqtick_graph_unfinished.argtypes = [C.c_void_p, C.c_uint64, abi.u64p, abi.u32p]
        self._chk(self._lib.hqtick_graph_unfinished(self._ctx, len(a), a.ctypes.data_as(abi.u64p), out.ctypes.data_as(abi.u32p)))
        return out

    def resident_check(self, parts: int = abi.HQ_CHECK_ALL) -> dict:
        """hqtick_resident_check: the audit of everything resident, on the device (abi.parse_check_report: checked, n_failed, count / first per invariant name, failed)"""
        self._lib.hqtick_resident_check.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(abi.CheckReportC)]
        r = abi.CheckReportC()
        self._chk(self._lib.hqtick_resident_check(self._ctx, parts, C.byref(r)))
        return abi.parse_check_report(r)

    def graph_stats(self) -> dict:
        st = abi.GraphStatsC()
        self._lib.hqtick_graph_get_stats.argtypes = [C.c_void_p, C.POINTER(abi.GraphStatsC)]
        self._chk(self._lib.hqtick_graph_get_stats(self._ctx, C.byref(st)))
        return {k: getattr(st, k) for k, _ in abi.GraphStatsC._fields_}

    def query(self, snap: abi.Snapshot, fake_ids, fake_total, fake_remaining=None, fake_min_util=None):
        sc = snap.to_c()
        n = len(fake_ids)
        ids = np.ascontiguousarray(fake_ids, np.uint32)
        tot = np.ascontiguousarray(np.asarray(fake_total, np.uint64).reshape(-1))
        rem = np.ascontiguousarray(fake_remaining if fake_remaining is not None else np.full(n, abi.HQ_NO_TIME_LIMIT), np.int64)
        mu = np.ascontiguousarray(fake_min_util if fake_min_util is not None else np.zeros(n), np.float32)
        q = abi.QueryWorkersC(n, ids.ctypes.data_as(abi.u32p), tot.ctypes.data_as(abi.u64p), rem.ctypes.data_as(abi.i64p), mu.ctypes.data_as(abi.f32p))
        out = abi.QueryResultC()
        rc = self._lib.hqtick_query(self._ctx, C.byref(sc), C.byref(q), C.byref(out))
        if rc < 0:
            raise HqTickError(rc, self._err())
        return abi._np(out.is_loaded, n, np.uint8).astype(bool), bool(out.is_optimal)

    def query_resident(self, snap: abi.Snapshot, fake_ids, fake_total, fake_remaining=None, fake_min_util=None, resident_workers: bool = False):
        """hqtick_query_resident (ABI 11): the query on the resident ready set; `snap` supplies requests and prefill sets (its task columns are ignored).
        Returns (is_loaded per fake worker, is_optimal, rq_ready = live resident tasks per request).  resident_workers: the snapshot travels without its
        worker side (n_workers = HQ_WORKERS_RESIDENT), as a host on hqtick_cluster_* sends it."""
        sc = snap.to_c(resident_workers=resident_workers)
        n = len(fake_ids)
        ids = np.ascontiguousarray(fake_ids, np.uint32)
        tot = np.ascontiguousarray(np.asarray(fake_total, np.uint64).reshape(-1))
        rem = np.ascontiguousarray(fake_remaining if fake_remaining is not None else np.full(n, abi.HQ_NO_TIME_LIMIT), np.int64)
        mu = np.ascontiguousarray(fake_min_util if fake_min_util is not None else np.zeros(n), np.float32)
        q = abi.QueryWorkersC(n, ids.ctypes.data_as(abi.u32p), tot.ctypes.data_as(abi.u64p), rem.ctypes.data_as(abi.i64p), mu.ctypes.data_as(abi.f32p))
        out = abi.QueryResultC()
        Q = len(snap.requests)
        rq_ready = np.zeros(max(Q, 1), np.uint64)
        rc = self._lib.hqtick_query_resident(self._ctx, C.byref(sc), C.byref(q), C.byref(out), rq_ready.ctypes.data_as(abi.u64p))
        if rc < 0:
            raise HqTickError(rc, self._err())
        return abi._np(out.is_loaded, n, np.uint8).astype(bool), bool(out.is_optimal), rq_ready[:Q].copy()

    def time_kernel(self, which: int, iters: int = 100) -> float:
        """hqtick_time_kernel (measurement library only: Tick(..., measure=True)): average duration (us) of `iters` back-to-back launches of K1 (0) / K4 (1)."""
        us = C.c_double()
        self._lib.hqtick_time_kernel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        rc = self._lib.hqtick_time_kernel(self._ctx, which, iters, C.byref(us))
        if rc < 0:
            raise HqTickError(rc, self._err())
        return us.value

    def set_kernel_timing(self, on):
        """False / True: every measured kernel; 2: K1 (k_level_hist) alone"""
        self._lib.hqtick_set_kernel_timing.argtypes = [C.c_void_p, C.c_int]
        self._chk(self._lib.hqtick_set_kernel_timing(self._ctx, 2 if on == 2 else (1 if on else 0)))

    def kernel_stats(self) -> dict:
        ks = abi.KernelStatsC()
        self._lib.hqtick_kernel_stats_last(self._ctx, C.byref(ks))
        return {f: getattr(ks, f) for f, _ in abi.KernelStatsC._fields_}
