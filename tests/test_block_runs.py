"""Equal-block runs of the coupled model (csrc/milp.h: Model::block_runs): consecutive worker blocks that differ in their costs only are built in one go
(csrc/host_model.cpp) and flattened once (csrc/price.cpp).  The contract is that NOTHING moves: with the runs on and off the model and everything the
flattener makes of it are equal byte for byte (64-bit FNV-1a digests over every array, hqtick_debug_last_coupled_digest), and so are the tick's results and
the number of sweeps.  Every case also states how many blocks it expects the runs to cover, so that a path that switched itself off cannot pass.
Host stages with the emulated sweeps: runs without a GPU (tests/test_gpu_block_runs.py runs the same comparison through k_price_sweep)."""
import ctypes as C

import numpy as np
import pytest

from host_stages import HostStages
from hyperqueue_amd import abi, workloads
from hyperqueue_amd.core import priority_from_user

FR = 10_000  # ResourceAmount fractions per unit


def _lib(hs):
    lib = hs.lib
    lib.hqtick_debug_set_price_emulation.argtypes = [C.c_int, C.c_uint32]
    lib.hqtick_debug_last_price.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.hqtick_debug_set_block_runs.argtypes = [C.c_int]
    lib.hqtick_debug_corrupt_block_runs.argtypes = [C.c_int]
    lib.hqtick_debug_check_model_hints.argtypes = [C.c_int]
    lib.hqtick_debug_last_coupled_digest.argtypes = [C.POINTER(C.c_uint64)]
    return lib


def tick(snap, runs: int, corrupt: bool = False):
    """one tick's host stages -> (result, (model digest, tables digest, runs recorded, blocks covered), sweeps, rounds, hint mismatches)"""
    hs = HostStages(abi.make_config(time_limit_s=5.0))
    lib = _lib(hs)
    lib.hqtick_debug_set_price_emulation(1, 64)
    lib.hqtick_debug_set_block_runs(runs)
    lib.hqtick_debug_corrupt_block_runs(1 if corrupt else 0)
    lib.hqtick_debug_check_model_hints(1)  # everything a run passed over is flattened block by block as well, and compared
    try:
        got = hs.stages(snap)
        mism = lib.hqtick_debug_model_hint_mismatches()
    finally:
        lib.hqtick_debug_set_price_emulation(0, 0)
        lib.hqtick_debug_corrupt_block_runs(0)
        lib.hqtick_debug_check_model_hints(0)
        lib.hqtick_debug_set_block_runs(-1)
    d = (C.c_uint64 * 4)()
    lib.hqtick_debug_last_coupled_digest(d)
    sw, rd = C.c_uint32(), C.c_uint32()
    lib.hqtick_debug_last_price(C.byref(sw), C.byref(rd))
    return got, tuple(int(v) for v in d), sw.value, rd.value, mism


def four_levels(snap):
    """a fourth priority level: every 20th task of the ready set"""
    prio = np.array(snap.task_priority, np.uint64)
    prio[::20] = priority_from_user(3)
    snap.task_priority = prio
    return snap


def c3p(W, tasks_per_worker=2500, name="c3p"):
    return workloads.make(name, n_tasks=W * tasks_per_worker, n_workers=W)


def halves(W):
    snap = c3p(W)
    free = np.array(snap.worker_free, np.uint64).reshape(W, -1)
    free[W // 2:, 0] -= 16 * FR  # the upper half has 16 cpus less to give
    snap.worker_free = free
    return snap


def every_third_busy(W):
    """workers 0, 3, 6, ... run one 4-cpu task: singles, and runs of two between them"""
    snap = c3p(W)
    free = np.array(snap.worker_free, np.uint64).reshape(W, -1)
    assigned = [[] for _ in range(W)]
    for w in range(0, W, 3):
        free[w, 0] -= 4 * FR
        assigned[w] = [(1, 0)]
    snap.worker_free, snap.assigned = free, assigned
    return snap


def one_min_utilization(W):
    snap = c3p(W)
    mu = np.zeros(W, np.float32)
    mu[W // 2] = 0.5
    snap.worker_min_utilization = mu
    return snap


def one_unbounded(W):
    """worker W // 2 has no limit on mem: its mem terms are carried into the next worker's row, and neither block is a plain one"""
    snap = c3p(W)
    free, total = np.array(snap.worker_free, np.uint64).reshape(W, -1), np.array(snap.worker_total, np.uint64).reshape(W, -1)
    free[W // 2, 2] = total[W // 2, 2] = abi.HQ_AMOUNT_MAX
    snap.worker_free, snap.worker_total = free, total
    return snap


def few_tasks(W, n_tasks):
    """one level, far fewer tasks than the workers hold: the lazy batch-size rows fail, the model is coupled, and the workers that no optimum uses are
    left out of it (host_model.cpp: worker_off) — the last ones of the one class, behind the run's members (worker_off exists on ticks without cuts only)"""
    return workloads.make("c3", n_tasks=n_tasks, n_workers=W)


def kept_workers(snap, got):
    """host_model.cpp's bound on the workers an optimum uses: min(#tasks, 1 + sum_e (D_e - 1) / (free_e - dmax_e)), identical workers, one variant per request"""
    W = len(snap.worker_id)
    free = [int(v) for v in np.array(snap.worker_free, np.uint64).reshape(W, -1)[0]]
    D, dmax, n = [0] * len(free), [0] * len(free), 0
    for b in got.batches:
        n += b.size
        for r, _kind, a in snap.requests[b.rq][0]["entries"]:
            D[r] += a * b.size
            dmax[r] = max(dmax[r], a)
    k = 1 + sum((D[r] - 1) // (free[r] - dmax[r]) for r in range(len(free)) if dmax[r] and D[r] > 0)
    return min(n, k, W)


def busy(W=96, n_tasks=3000):
    """a cluster mid-run (few enough ready tasks that the lower priority levels, and with them the cuts, come into play)"""
    return workloads.make_steady("c3p", n_tasks=n_tasks, n_workers=W)


# (name, snapshot, runs the builder records, blocks the flattener takes from a run's first block, does the model reach the sweeps' tables at all)
CASES = [
    ("identical_16", lambda: c3p(16), 1, 16, True),
    ("identical_64_four_levels", lambda: four_levels(c3p(64)), 1, 64, True),
    ("two_halves", lambda: halves(32), 2, 32, True),
    ("every_third_busy", lambda: every_third_busy(32), 10, 20, True),  # 0 | 1 2 | 3 | 4 5 | ... | 28 29 | 30 | 31: ten pairs, worker 31 follows 30 alone
    # runs 0..15 and 17..31 — and worker 16's block has a 0/1 column and a `>=` row: not a packing, which keeps the WHOLE model off the tables (with or without runs)
    ("min_utilization_inside", lambda: one_min_utilization(32), 2, 0, False),
    # runs 0..15 and 18..31: worker 16's mem terms are carried into worker 17's row, so neither block is a plain one; the flattener refuses the whole model
    # ("shared list that is not a wide left-hand side"), with or without runs
    ("unbounded_inside", lambda: one_unbounded(32), 2, 0, False),
    ("c4_or_lists_64", lambda: c3p(64, name="c4p"), 1, 64, True),
    ("busy_96", busy, 0, 0, True),
]


@pytest.mark.parametrize("name,make,want_runs,want_covered,tables", CASES, ids=[c[0] for c in CASES])
def test_runs_change_nothing(name, make, want_runs, want_covered, tables):
    snap = make()
    on, d_on, sw_on, rd_on, mism_on = tick(snap, 1)
    off, d_off, sw_off, rd_off, mism_off = tick(snap, 0)
    print(name, "on", [hex(v) for v in d_on[:2]], d_on[2:], sw_on, rd_on, "off", [hex(v) for v in d_off[:2]], d_off[2:], sw_off, rd_off)
    assert mism_on == 0 and mism_off == 0
    assert d_off[2] == 0 and d_off[3] == 0, "runs recorded with the switch off"
    assert d_on[0] != 0 and d_on[0] == d_off[0], "the model differs"
    assert d_on[1] == d_off[1] and (d_on[1] != 0) == tables, "the flattened problem differs"
    assert (on.status, on.is_optimal, on.batches, on.counts) == (off.status, off.is_optimal, off.batches, off.counts)
    assert (sw_on, rd_on) == (sw_off, rd_off)
    assert d_on[2] == want_runs
    assert d_on[3] == want_covered


def test_the_busy_cluster_is_one_free_vector_per_worker():
    """what makes busy_96 the case where every run has length 1: no two neighbours share their rows"""
    snap = busy()
    W = len(snap.worker_id)
    free = np.array(snap.worker_free, np.uint64).reshape(W, -1).tolist()
    assert all(free[w] != free[w + 1] or snap.assigned[w] != snap.assigned[w + 1] for w in range(W - 1))


def test_workers_left_out_do_not_break_a_run():
    snap = few_tasks(64, 600)
    on, d_on, sw_on, rd_on, mism = tick(snap, 1)
    off, d_off, sw_off, rd_off, _ = tick(snap, 0)
    kept = kept_workers(snap, on)
    print("kept", kept, d_on, d_off)
    assert 8 <= kept < 64, "the case must leave workers out and still have the eight blocks the tables ask for"
    assert mism == 0 and d_on[0] == d_off[0] and d_on[1] == d_off[1] and d_on[1] != 0
    assert d_on[2] == 1 and d_on[3] == kept
    assert (on.status, on.is_optimal, on.batches, on.counts, sw_on, rd_on) == (off.status, off.is_optimal, off.batches, off.counts, sw_off, rd_off)


def test_a_false_run_is_refused():
    """two neighbouring runs merged into one claim: the blocks differ in their bounds and right-hand sides, the flattener's comparison fails, the claimed
    blocks are flattened one by one — the same tables — and the runs it was not lied to about still count"""
    snap = halves(32)
    good, d_good, sw_good, _, _ = tick(snap, 1)
    bad, d_bad, sw_bad, _, mism = tick(snap, 1, corrupt=True)
    off, d_off, sw_off, _, _ = tick(snap, 0)
    assert d_good[2] == 2 and d_good[3] == 32
    assert d_bad[2] == 1 and d_bad[3] == 0, "the false run was taken"
    assert mism == 0
    assert d_bad[0] == d_off[0] and d_bad[1] == d_off[1] and d_bad[1] != 0
    assert (bad.status, bad.is_optimal, bad.batches, bad.counts, sw_bad) == (off.status, off.is_optimal, off.batches, off.counts, sw_off)
