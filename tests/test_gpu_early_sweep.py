"""The zero-price sweep launched from inside the flattening, on the block tables alone (csrc/price.h: Sweeper::begin_blocks / begin_wide; csrc/price.hip) — GPU only.
k_price_sweep runs with K = 0 on an all-zero col_woff while the host builds the wide rows' tables, which follow it on the stream; the host adds the first cut's
activities up from the patterns in pinned memory.  One context per order in turn, same process: the same counts, records, free resources and number of sweeps, both
certified.  (tests/test_early_sweep.py compares tables and the first cut byte for byte on the CPU.)"""
import ctypes as C
import functools

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads
from hyperqueue_amd.tick import Tick

pytestmark = pytest.mark.gpu

# A: 256 blocks, 2048 block columns, 1 sweep.  B: 87 wide rows, 14 flags, 3072 conditional bounds (re-sweeps at zero prices under other bounds), ~212 sweeps.
SHAPES = {"A": dict(n_tasks=400_000, n_workers=256), "B": dict(n_tasks=600, n_workers=256)}


@functools.lru_cache(maxsize=None)
def _snap(shape):
    return workloads.make("c3p", **SHAPES[shape])


def _hooks(t):
    lib = t._lib
    lib.hqtick_debug_set_early_sweep.argtypes = [C.c_int]
    lib.hqtick_debug_early_sweeps.restype = C.c_uint32
    return lib


def _tick(snap, early, flags=0, repeat=1, resident=False):
    t = Tick(abi.make_config(time_limit_s=5.0, flags=flags), measure=True)  # libhqtick_test.so: the product's objects plus the hooks
    lib = _hooks(t)
    lib.hqtick_debug_set_early_sweep(early)
    try:
        if resident:
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            t.cluster_upload(snap.to_c())
        out = []
        for _ in range(repeat):
            res = t.tick(snap, resident=resident)
            out.append((res, t.kernel_stats()["price_sweeps"]))
        n_early = lib.hqtick_debug_early_sweeps()
    finally:
        lib.hqtick_debug_set_early_sweep(-1)
        t.close()
    return out, n_early


def _same(a, b):
    assert (a.status, a.is_optimal, a.is_canonical) == (b.status, b.is_optimal, b.is_canonical)
    assert a.batches == b.batches and a.counts == b.counts
    assert a.records == b.records and a.retracts == b.retracts
    assert np.array_equal(a.new_free, b.new_free)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_a_device_tick_is_the_same_in_both_orders(shape):
    snap = _snap(shape)
    (late, sw_late), = _tick(snap, 0)[0]
    ((early, sw_early),), n_early = _tick(snap, 1)
    print(shape, "sweeps", sw_early, sw_late)
    assert n_early == 1, "the sweep was not launched from the flattener"
    assert late.status == abi.HQTICK_DONE and late.is_optimal and early.status == abi.HQTICK_DONE and early.is_optimal
    assert sw_late > 0 and sw_early == sw_late
    _same(early, late)


def test_the_cold_resident_tick_repeated():
    """bench.py's pattern: one context, resident inputs, HQTICK_FLAG_NO_TICK_CACHES, the same tick five times — every early launch reuses the sweeper's buffers
    behind the sweeps of the tick before"""
    snap = _snap("A")
    (late, sw_late), = _tick(snap, 0, flags=abi.HQTICK_FLAG_NO_TICK_CACHES, resident=True)[0]
    out, n_early = _tick(snap, 1, flags=abi.HQTICK_FLAG_NO_TICK_CACHES, repeat=5, resident=True)
    assert n_early == 5
    assert late.status == abi.HQTICK_DONE and late.is_optimal
    for i, (res, sw) in enumerate(out):
        assert sw == sw_late and sw > 0, (i, sw, sw_late)
        _same(res, late)
