"""Equal-block runs of the coupled model (csrc/milp.h: Model::block_runs) on the device — GPU only.  The smallest shapes that take the fast path to
k_price_sweep (at least 2048 model columns and 8 blocks: 256 workers of c3p): one tick with the runs on and one with them off, in the same process,
must give the same result in every array, walk the same number of sweeps and come out DONE and certified.  (tests/test_block_runs.py compares the model
and the tables byte for byte on the CPU; the digests are compared here as well, since the test library carries them.)"""
import ctypes as C

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads
from hyperqueue_amd.tick import Tick

pytestmark = pytest.mark.gpu

FR = 10_000


def _identical():
    return workloads.make("c3p", n_tasks=400_000, n_workers=256)


def _upper_half_changed():
    snap = _identical()
    free = np.array(snap.worker_free, np.uint64).reshape(256, -1)
    free[128:, 0] -= 16 * FR
    snap.worker_free = free
    return snap


def _tick(snap, runs):
    t = Tick(abi.make_config(time_limit_s=5.0), measure=True)  # libhqtick_test.so: the product's objects plus the hooks
    lib = t._lib
    lib.hqtick_debug_set_block_runs.argtypes = [C.c_int]
    lib.hqtick_debug_last_coupled_digest.argtypes = [C.POINTER(C.c_uint64)]
    lib.hqtick_debug_set_block_runs(runs)
    try:
        res = t.tick(snap)
        ks = t.kernel_stats()
    finally:
        lib.hqtick_debug_set_block_runs(-1)
        t.close()
    d = (C.c_uint64 * 4)()
    lib.hqtick_debug_last_coupled_digest(d)
    return res, ks, tuple(int(v) for v in d)


@pytest.mark.parametrize("make,want_runs", [(_identical, 1), (_upper_half_changed, 2)], ids=["identical_256", "upper_half_changed_256"])
def test_a_device_tick_is_the_same_with_and_without_runs(make, want_runs):
    snap = make()
    on, ks_on, d_on = _tick(snap, 1)
    off, ks_off, d_off = _tick(snap, 0)
    print("on", d_on, ks_on["price_sweeps"], "off", d_off, ks_off["price_sweeps"])
    assert on.status == abi.HQTICK_DONE and on.is_optimal and off.status == abi.HQTICK_DONE and off.is_optimal
    assert ks_on["price_sweeps"] > 0 and ks_on["price_sweeps"] == ks_off["price_sweeps"] and ks_on["price_rounds"] == ks_off["price_rounds"]
    assert d_on[2] == want_runs and d_on[3] == 256 and d_off[2] == 0 and d_off[3] == 0
    assert d_on[0] == d_off[0] and d_on[1] == d_off[1] and d_on[1] != 0
    assert (on.status, on.is_optimal, on.is_canonical) == (off.status, off.is_optimal, off.is_canonical)
    assert on.batches == off.batches and on.counts == off.counts
    assert on.records == off.records and on.retracts == off.retracts
    assert on.redirects == off.redirects and on.redirect_kinds == off.redirect_kinds and on.mn == off.mn
    assert np.array_equal(on.new_free, off.new_free)
