"""The coupled fast path's row check run while phase C's kernels do (csrc/hqtick.cpp: TickRun::run, csrc/map.h: PhaseC::while_gpu_runs) — GPU only.
The check changes nothing in the point, so the tick with the deferral on and off must be the same in every parsed field; a deferred check that fails makes the tick
discard the phase C it has just waited for and come back with the classic path's placement, and nothing of the discarded pass survives into the next tick — the
two-call form's hqtick_ready_consume_last included.  Where a discarded phase C would leave a trace the tick never defers.  (tests/test_deferred_row_check.py runs
the solver side on the CPU.)

The workload is the smallest c3p shape the fast path takes: 256 workers x 8 classes = 2048 block columns (FAST_MIN_COLS), three levels, and 20 000 ready tasks, of
which the first tick hands out the larger part: the second tick of a context still has work.  The classic tick is a context under hqtick_debug_set_fast_path(0):
what HQMILP_FAST=0 does, for one thread — the environment variable itself is read once per process, at the first coupled solve.  The armed failure is a host-side boolean: no test here provokes a device fault."""
import ctypes as C
import functools

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads
from hyperqueue_amd.tick import Tick

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _snap():
    return workloads.make("c3p", n_workers=256, n_tasks=20_000)


def _hooks(t):
    lib = t._lib
    lib.hqtick_debug_set_fast_path.argtypes = [C.c_int]
    lib.hqtick_debug_set_defer_row_check.argtypes = [C.c_int]
    lib.hqtick_debug_deferred_row_checks.argtypes = [C.c_int]
    lib.hqtick_debug_deferred_row_checks.restype = C.c_uint32
    lib.hqtick_debug_fail_row_checks.argtypes = [C.c_uint32]
    lib.hqtick_debug_fail_row_checks.restype = C.c_uint32
    return lib


def _same(a, b):
    assert (a.status, a.is_optimal, a.is_canonical) == (b.status, b.is_optimal, b.is_canonical)
    assert a.batches == b.batches and a.counts == b.counts
    assert a.records == b.records and a.retracts == b.retracts
    assert np.array_equal(a.new_free, b.new_free)


def two_ticks(defer, fail=0, fast=-1):
    """one context, resident inputs, the two-call form twice: tick, hqtick_ready_consume_last, tick, hqtick_ready_consume_last.  `fail` and `fast` hold for the first
    tick only.  -> per tick (result, price sweeps, deferred checks, live ready tasks after the consume), and the armed failures left unused"""
    snap = _snap()
    t = Tick(abi.make_config(time_limit_s=5.0), measure=True)  # libhqtick_test.so: the product's objects plus the hooks
    lib = _hooks(t)
    lib.hqtick_debug_set_defer_row_check(defer)
    lib.hqtick_debug_set_fast_path(fast)
    lib.hqtick_debug_fail_row_checks(fail)
    lib.hqtick_debug_deferred_row_checks(1)
    out, unused = [], None
    try:
        t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
        t.cluster_upload(snap.to_c())
        for i in range(2):
            res = t.tick(snap, resident=True)
            sweeps, n = t.kernel_stats()["price_sweeps"], lib.hqtick_debug_deferred_row_checks(1)
            if i == 0:
                unused = lib.hqtick_debug_fail_row_checks(0)
                lib.hqtick_debug_set_fast_path(-1)
            t.ready_consume_last()
            out.append((res, sweeps, n, t.ready_count()))
    finally:
        lib.hqtick_debug_fail_row_checks(0)
        lib.hqtick_debug_set_fast_path(-1)
        lib.hqtick_debug_set_defer_row_check(-1)
        t.close()
    return out, unused


@functools.lru_cache(maxsize=None)
def _inline():
    """today's order: the reference of the comparisons, computed once"""
    return two_ticks(0)[0]


def test_the_tick_is_the_same_with_the_check_inline_and_deferred():
    off, on = _inline(), two_ticks(1)[0]
    for i, ((r_off, sw_off, n_off, live_off), (r_on, sw_on, n_on, live_on)) in enumerate(zip(off, on)):
        print("tick", i, "sweeps", sw_on, sw_off, "deferred checks", n_on, n_off, "live", live_on, live_off)
        assert r_off.status == abi.HQTICK_DONE and r_off.is_optimal
        if i == 0:
            assert sw_off > 0, "the workload must take the fast path"
            assert 0 < live_off < len(_snap().task_id), "the first tick must hand out some of the tasks and leave some"
        # (the second tick's model may be below the fast path's size: the classic path sweeps too, so its sweeps say nothing about a pending check)
        assert n_off == 0 and (n_on == 1 if i == 0 else n_on <= 1)
        assert sw_on == sw_off and live_on == live_off
        _same(r_on, r_off)
    assert sum(len(r) for r in off[0][0].records) > 0


def test_a_failing_check_gives_the_classic_tick_and_leaves_nothing_behind():
    classic, _ = two_ticks(0, fast=0)
    failed, unused = two_ticks(1, fail=1)
    (r_c, sw_c, n_c, live_c), (r_f, sw_f, n_f, live_f) = classic[0], failed[0]
    print("sweeps classic", sw_c, "after the failed check", sw_f, "live", live_c, live_f)
    assert n_c == 0 and n_f == 1 and unused == 0, "the first tick's check was not deferred, or did not consume the armed failure"
    _same(r_f, r_c)
    assert live_f == live_c   # hqtick_ready_consume_last replayed the SECOND pass's selection
    # the next tick on the same context: the plain one, on the same state
    (r_c2, sw_c2, _, live_c2), (r_f2, sw_f2, n_f2, live_f2) = classic[1], failed[1]
    assert n_f2 <= 1 and sw_f2 == sw_c2
    _same(r_f2, r_c2)
    assert live_f2 == live_c2


@pytest.mark.parametrize("what", ["consume_in_tick", "sink", "ledger"])
def test_no_deferral_where_a_discarded_phase_c_would_leave_a_trace(what):
    snap = _snap()
    flags = abi.HQTICK_FLAG_CONSUME_IN_TICK if what == "consume_in_tick" else 0
    t = Tick(abi.make_config(time_limit_s=5.0, flags=flags), measure=True)
    lib = _hooks(t)
    lib.hqtick_debug_set_defer_row_check(1)
    lib.hqtick_debug_deferred_row_checks(1)
    sink = None
    try:
        t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
        t.cluster_upload(snap.to_c())
        if what == "sink":
            import torch

            from hyperqueue_amd.sharded import sink_layout

            sink = torch.zeros(sink_layout(len(snap.worker_id), 32768)[4], dtype=torch.uint8, device="cuda")
            assert t.set_record_sink(sink, len(snap.worker_id)) >= 32768
        sc = snap.to_c(resident_workers=what == "ledger")
        if what == "ledger":
            t.assigned_enable([])
            sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
        res = t.tick_raw(sc, resident=True)   # (with a sink the records stay in HBM: nothing to parse)
        n = lib.hqtick_debug_deferred_row_checks(1)
        sweeps = t.kernel_stats()["price_sweeps"]
        print(what, "sweeps", sweeps, "deferred checks", n)
        assert res.status == abi.HQTICK_DONE and sweeps > 0, "the tick must take the fast path"
        assert n == 0
        if what == "sink":
            t.set_record_sink(None)
    finally:
        lib.hqtick_debug_set_defer_row_check(-1)
        t.close()
