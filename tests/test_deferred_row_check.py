"""The coupled fast path's last step — the certified point against every row and bound of the model, then the certificate on the rounded point's objective
(csrc/milp.cpp: check_point) — may leave the solver pending (hqmilp::SolveOpts::defer_row_check) and be run by the caller; the tick runs it while phase C's kernels do
(tests/test_gpu_deferred_row_check.py).  Here: the host stages with the emulated sweeps, which run the check right behind the solver when
hqtick_debug_set_defer_row_check(1) allows it.  The contract is that nothing moves: the same status, counts, sweeps and rounds with the check inline and deferred,
and a deferred check that fails gives what the same call gives with the fast path off, in every field.

The models of tests/coupled_cases.py have at most 600 columns and the fast path starts at 2048 (FAST_MIN_COLS), so none of them gets there: they pin that a model
the fast path does not take has nothing pending (the counter says which did).  The two c3p shapes of tests/test_early_sweep.py do take it."""
import ctypes as C
import functools

import pytest

import coupled_cases as cc
from host_stages import HostStages
from hyperqueue_amd import abi, workloads

# A: 256 blocks, 2048 block columns, 1 sweep.  B: 87 wide rows, 14 flags, 212 sweeps (tests/test_early_sweep.py)
SHAPES = {"A": dict(n_tasks=400_000, n_workers=256), "B": dict(n_tasks=600, n_workers=256)}
# (seed 2000 of every variant that has it: these solve in well under a second.  mu6's three seeds and seed 2005 run into the time limit, where two runs of the same
# call need not agree)
COUPLED = [(v, 2000) for v in cc.VARIANTS if 2000 in cc.GPU_SEEDS[v]]


def _lib(hs):
    lib = hs.lib
    lib.hqtick_debug_set_price_emulation.argtypes = [C.c_int, C.c_uint32]
    lib.hqtick_debug_last_price.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.hqtick_debug_set_fast_path.argtypes = [C.c_int]
    lib.hqtick_debug_set_defer_row_check.argtypes = [C.c_int]
    lib.hqtick_debug_deferred_row_checks.argtypes = [C.c_int]
    lib.hqtick_debug_deferred_row_checks.restype = C.c_uint32
    lib.hqtick_debug_fail_row_checks.argtypes = [C.c_uint32]
    lib.hqtick_debug_fail_row_checks.restype = C.c_uint32
    return lib


@functools.lru_cache(maxsize=None)
def _snap(kind, key):
    return workloads.make("c3p", **SHAPES[key]) if kind == "c3p" else cc.case(kind, key)


def stages(kind, key, defer, fail=0, fast=-1):
    """one call of the host stages -> (every field the callers of the solver see, deferred checks counted during the call, armed failures left unused)"""
    hs = HostStages(abi.make_config(time_limit_s=5.0))
    lib = _lib(hs)
    lib.hqtick_debug_set_price_emulation(1, 0)
    lib.hqtick_debug_set_fast_path(fast)
    lib.hqtick_debug_set_defer_row_check(defer)
    lib.hqtick_debug_fail_row_checks(fail)
    lib.hqtick_debug_deferred_row_checks(1)
    try:
        got = hs.stages(_snap(kind, key))
        n_deferred = lib.hqtick_debug_deferred_row_checks(1)
        mn = cc.last_mn(lib)
    finally:
        unused = lib.hqtick_debug_fail_row_checks(0)
        lib.hqtick_debug_set_defer_row_check(-1)
        lib.hqtick_debug_set_fast_path(-1)
        lib.hqtick_debug_set_price_emulation(0, 0)
    sw, rd = C.c_uint32(), C.c_uint32()
    lib.hqtick_debug_last_price(C.byref(sw), C.byref(rd))
    return dict(status=got.status, is_optimal=got.is_optimal, is_canonical=got.is_canonical, batches=got.batches, counts=got.counts, mn=mn, sweeps=sw.value,
                rounds=rd.value), n_deferred, unused


@functools.lru_cache(maxsize=None)
def _inline(kind, key):
    """today's order: the reference of every comparison, computed once"""
    got, n, _ = stages(kind, key, 0)
    assert n == 0
    return got


@pytest.mark.parametrize("shape,want_sweeps", [("A", 1), ("B", 212)])
def test_the_deferred_check_changes_nothing(shape, want_sweeps):
    inline = _inline("c3p", shape)
    deferred, n, _ = stages("c3p", shape, 1)
    print(shape, "sweeps", deferred["sweeps"], inline["sweeps"], "rounds", deferred["rounds"], inline["rounds"], "deferred checks", n)
    assert inline["status"] == abi.HQTICK_DONE and inline["is_optimal"] and inline["sweeps"] == want_sweeps, "the shape must take the fast path and certify"
    assert n == 1, "the check did not leave the solver pending"
    assert deferred == inline


@pytest.mark.parametrize("variant,seed", COUPLED)
def test_coupled_cases_allowed_and_forbidden(variant, seed):
    inline = _inline(variant, seed)
    deferred, n, _ = stages(variant, seed, 1)
    print(variant, seed, "sweeps", inline["sweeps"], "deferred checks", n)
    assert deferred == inline
    assert n == 0, "a model below the fast path's size left a check pending"   # (see the module's docstring: none of these models reaches it)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_a_failing_check_gives_the_classic_answer(shape):
    """(on these shapes the classic path reaches the same placement as the sweeps, so the answer alone cannot tell that the second solve ran: the counters say
    that a check was pending and that it consumed the armed failure)"""
    classic, n0, _ = stages("c3p", shape, 0, fast=0)
    failed, n, unused = stages("c3p", shape, 1, fail=1)
    print(shape, "sweeps classic", classic["sweeps"], "after the failed check", failed["sweeps"])
    assert n0 == 0 and n == 1 and unused == 0
    assert failed == classic
    again, n, _ = stages("c3p", shape, 1)   # the next call is the plain one
    assert n == 1 and again == _inline("c3p", shape)


@pytest.mark.parametrize("switch", [-1, 0])
def test_a_caller_that_does_not_ask_sees_nothing_pending(switch):
    """the host stages set Problem::defer_row_check only while the switch is 1; an armed failure stays armed, because no deferred check runs"""
    got, n, unused = stages("c3p", "A", switch, fail=1)
    assert n == 0 and unused == 1
    assert got == _inline("c3p", "A")
