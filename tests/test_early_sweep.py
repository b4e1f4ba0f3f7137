"""The first sweep of a coupled solve runs at zero prices, where a block's reduced costs are its costs: it is launched from inside the flattening, as soon as the
block tables are final, on those tables alone (csrc/price.h: Sweeper::begin_blocks / begin_wide), and the wide rows' activities of its patterns are added up on the
host.  The contract is that NOTHING moves: with the early launch on and off the tables, the first cut (every byte of it), the number of sweeps and rounds and the
tick's answer are equal.  Host stages with the emulated sweeps, which walk the same order as the device: the early sweep runs with K = 0 on an all-zero col_woff
BEFORE the wide rows' tables exist (tests/test_gpu_early_sweep.py runs the comparison through k_price_sweep)."""
import ctypes as C
import functools

import pytest

from host_stages import HostStages
from hyperqueue_amd import abi, workloads


def _lib(hs):
    lib = hs.lib
    lib.hqtick_debug_set_price_emulation.argtypes = [C.c_int, C.c_uint32]
    lib.hqtick_debug_last_price.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.hqtick_debug_set_block_runs.argtypes = [C.c_int]
    lib.hqtick_debug_last_coupled_digest.argtypes = [C.POINTER(C.c_uint64)]
    lib.hqtick_debug_set_early_sweep.argtypes = [C.c_int]
    lib.hqtick_debug_early_sweeps.restype = C.c_uint32
    lib.hqtick_debug_capture_first_cut.argtypes = [C.c_int]
    lib.hqtick_debug_first_cut.argtypes = [C.c_char_p, C.c_uint32]
    lib.hqtick_debug_first_cut.restype = C.c_uint32
    lib.hqtick_debug_set_price_fault.argtypes = [C.c_int]
    return lib


# A: 256 blocks, 2048 block columns, 10 flags, 1 sweep.  B: 87 wide rows, 14 flags, 3072 conditional bounds, 212 sweeps; its wide rows tighten 512 column bounds, so
# it also pins that the bounds are final at the launch point.
SHAPES = {"A": dict(n_tasks=400_000, n_workers=256), "B": dict(n_tasks=600, n_workers=256)}


@functools.lru_cache(maxsize=None)
def _snap(shape):
    return workloads.make("c3p", **SHAPES[shape])


def tick(shape, early, runs=1, fault=-1):
    """one tick's host stages -> dict of everything the two orders must agree in, plus the early launches counted"""
    hs = HostStages(abi.make_config(time_limit_s=5.0))
    lib = _lib(hs)
    lib.hqtick_debug_set_price_emulation(1, 0)
    lib.hqtick_debug_set_block_runs(runs)   # (also installs the probe the digests are read from)
    lib.hqtick_debug_set_early_sweep(early)
    lib.hqtick_debug_capture_first_cut(1)
    lib.hqtick_debug_set_price_fault(fault)
    try:
        got = hs.stages(_snap(shape))
        n_early = lib.hqtick_debug_early_sweeps()
        size = lib.hqtick_debug_first_cut(None, 0)
        buf = C.create_string_buffer(max(size, 1))
        lib.hqtick_debug_first_cut(buf, size)
    finally:
        lib.hqtick_debug_set_price_fault(-1)
        lib.hqtick_debug_capture_first_cut(0)
        lib.hqtick_debug_set_early_sweep(-1)
        lib.hqtick_debug_set_block_runs(-1)
        lib.hqtick_debug_set_price_emulation(0, 0)
    d = (C.c_uint64 * 4)()
    lib.hqtick_debug_last_coupled_digest(d)
    sw, rd = C.c_uint32(), C.c_uint32()
    lib.hqtick_debug_last_price(C.byref(sw), C.byref(rd))
    return dict(status=got.status, is_optimal=got.is_optimal, batches=got.batches, counts=got.counts, sweeps=sw.value, rounds=rd.value,
                model=int(d[0]), tables=int(d[1]), cut=buf.raw[:size]), n_early


@functools.lru_cache(maxsize=None)
def _late(shape):
    """today's order: the reference of every comparison, computed once"""
    got, n_early = tick(shape, 0)
    assert n_early == 0
    return got


@pytest.mark.parametrize("shape,want_sweeps", [("A", 1), ("B", 212)])
def test_the_early_launch_changes_nothing(shape, want_sweeps):
    late = _late(shape)
    early, n_early = tick(shape, 1)
    print(shape, "sweeps", early["sweeps"], late["sweeps"], "rounds", early["rounds"], late["rounds"], "tables", hex(early["tables"]), hex(late["tables"]), "cut bytes", len(early["cut"]))
    assert n_early == 1, "the sweep was not launched from the flattener"
    assert late["status"] == abi.HQTICK_DONE and late["is_optimal"], "the shape must take the fast path and certify"
    assert late["sweeps"] == want_sweeps
    assert late["tables"] != 0 and early["tables"] == late["tables"] and early["model"] == late["model"]
    assert len(late["cut"]) > 8 * (2 + 16) and early["cut"] == late["cut"], "the first cut differs"
    assert (early["sweeps"], early["rounds"]) == (late["sweeps"], late["rounds"])
    assert (early["status"], early["is_optimal"], early["batches"], early["counts"]) == (late["status"], late["is_optimal"], late["batches"], late["counts"])


def test_without_block_runs():
    """HQMILP_BLOCK_RUNS=0's flattening (every block through the rows loop) with the early launch"""
    late = _late("A")
    early, n_early = tick("A", 1, runs=0)
    assert n_early == 1
    assert early["tables"] == late["tables"] and early["cut"] == late["cut"]
    assert {k: early[k] for k in ("status", "is_optimal", "batches", "counts", "sweeps", "rounds")} == {k: late[k] for k in ("status", "is_optimal", "batches", "counts", "sweeps", "rounds")}


@pytest.mark.parametrize("fault", [0, 1, 2])
def test_a_failing_sweeper(fault):
    """the sweeper refuses the model (0) or its first / second sweep fails: the tick returns what it returns in today's order — the host search takes the model — and
    the sweeper has been ended (the next tick on this thread sweeps again)"""
    late, _ = tick("A", 0, fault=fault)
    early, n_early = tick("A", 1, fault=fault)
    assert n_early == (1 if fault == 2 else 0)   # (a launch that failed, or tables that were refused, do not count)
    keys = ("status", "is_optimal", "batches", "counts", "sweeps", "rounds", "tables")
    assert {k: early[k] for k in keys} == {k: late[k] for k in keys}
    again, n_early = tick("A", 1)
    assert n_early == 1 and again == _late("A")
