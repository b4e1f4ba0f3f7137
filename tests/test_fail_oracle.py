"""SchedEnv.fail_tasks, the mirror's task_failed (server/reactor.rs:606-704): the scenarios of tests/fail_cases.py with the reference's outcomes, the decision rule
of hqtick_fail_tasks (csrc/fail_core.h through hqtick_debug_fail_kind) over the full table of its inputs against a restatement written here, what the random
histories of the GPU suite contain, and the new symbols in headers, libraries and bindings.  The CPU oracle is the scheduler where a scenario needs a tick.
No GPU needed."""
import collections
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import cancel_cases as cc
import fail_cases as fl
import finish_cases as fc
from hyperqueue_amd import abi, build, core
from hyperqueue_amd.core import SchedEnv
from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hqtick_fail_tasks", "hqtick_fail_last_routes", "hqtick_fail_last_consumers"]
K = abi
NO = abi.HQ_NO_WORKER
NAMES = ["NONE", "ASSIGNED", "MN", "PREFILLED", "RETRACTING", "WAITING", "REPEAT", "WRONG_WORKER", "NOT_WAITING", "GONE"]


@pytest.fixture(scope="module")
def backend():
    return Oracle(abi.make_config(reserve=1, fill_max=1, time_limit_s=20.0))


# ---------------------------------------------------------------------------------------------- the scenarios on the mirror alone
def test_running_task_on_error():
    e, ws, wf = fl.scenario_running_task_on_error()
    assert e.fail_tasks([(wf[2], ws[2])]) == 1
    fl.check_running_task_on_error(e, ws, wf)


def test_task_mn_fail():
    e, t1, root, other = fl.scenario_mn_fail()
    assert e.fail_tasks([(t1, other), (t1, NO), (t1, root), (t1, root), (t1, other)]) == 1
    assert e.last_fail_kinds == [K.HQ_FAIL_WRONG_WORKER, K.HQ_FAIL_NOT_WAITING, K.HQ_FAIL_MN, K.HQ_FAIL_REPEAT, K.HQ_FAIL_WRONG_WORKER]
    fl.check_mn_fail(e, t1)


def test_prefill_failed(backend):
    e, w1, tasks, t1, t2 = cc.setup_prefill(backend)
    assert e.finish_tasks([(t1, w1)]) == [] and e.last_finish_kinds == [K.HQ_FINISH_ASSIGNED]
    assert e.fail_tasks([(t2, w1)]) == 1
    fl.check_prefill_failed(e, w1, t1, t2)


def test_steal_failed(backend):
    e, w1, w2, t, on_w1 = fc.scenario_steal(backend)
    before = e.workers[w2].free[0]
    e.finish_tasks([(on_w1, w1)])
    assert e.fail_tasks([(t, w2)]) == 0 and e.last_fail_kinds == [K.HQ_FAIL_WRONG_WORKER] and t in e.redirects  # the target never got the task
    assert e.fail_tasks([(t, w1)]) == 1
    fl.check_steal_failed(e, w1, w2, t, before)


def test_worker_crashing_task_at_its_limit():
    e, w, t1 = fl.scenario_crash_limit()
    assert e.remove_worker(w) == [] and e.tasks[t1].state == core.WAITING and t1 in e.ready[e.tasks[t1].rq]  # back in its queue (reactor.rs:130-160)
    assert e.fail_tasks([(t1, w)]) == 0 and e.last_fail_kinds == [K.HQ_FAIL_NONE]
    assert e.fail_tasks([(t1, NO)]) == 1 and e.last_fail_kinds == [K.HQ_FAIL_WAITING]
    assert e.tasks[t1].state == core.FINISHED and all(t1 not in s for s in e.ready.values())


# ---------------------------------------------------------------------------------------------- the rule
def _debug_lib():
    build.build()
    lib = C.CDLL(build.TEST_LIB)
    lib.hqtick_debug_fail_kind.argtypes = [C.c_uint32] + [abi.u8p] * 8
    lib.hqtick_debug_fail_kind.restype = C.c_int
    return lib


def _rule(lib, rows):
    cols = [np.ascontiguousarray([r[k] for r in rows], np.uint8) for k in range(7)]
    out = np.full(len(rows), 255, np.uint8)
    assert lib.hqtick_debug_fail_kind(len(rows), *[c.ctypes.data_as(abi.u8p) for c in cols], out.ctypes.data_as(abi.u8p)) == len(rows)
    return out.tolist()


def _restated(found, cls, wm, of, om, none, earlier):
    """task_failed's arms (reactor.rs:622-669) as kinds, written from the reference and the header, not from fail_core.h"""
    if none:  # task_failed(None, ..): assert!(task.is_waiting()) -- a waiting task holds neither an entry nor a place in the Retracting table
        first = K.HQ_FAIL_NOT_WAITING if (found or of) else K.HQ_FAIL_WAITING
    elif of:  # TaskRuntimeState::Retracting { worker_id: w }: assert_eq!(worker_id, *w), whatever the ledger holds for the redirect target
        first = K.HQ_FAIL_RETRACTING if om else K.HQ_FAIL_WRONG_WORKER
    elif not found:
        first = K.HQ_FAIL_NONE
    elif not wm:
        first = K.HQ_FAIL_WRONG_WORKER
    else:
        first = {0: K.HQ_FAIL_ASSIGNED, 1: K.HQ_FAIL_MN, 2: K.HQ_FAIL_PREFILLED}[cls]
    return K.HQ_FAIL_REPEAT if earlier and first in K.HQ_FAIL_ACCEPTED else first


def test_the_rule_over_its_full_truth_table():
    lib = _debug_lib()
    assert [getattr(K, "HQ_FAIL_" + n) for n in NAMES] == list(range(10))
    assert K.HQ_FAIL_ACCEPTED == (1, 2, 3, 4, 5)
    rows = [(f, c, wm, of, om, none, earlier) for c in (0, 1, 2) for f, wm, of, om, none, earlier in itertools.product((0, 1), repeat=6)]
    assert len(set(rows)) == 192
    got = _rule(lib, rows)
    assert got == [_restated(*r) for r in rows]
    assert set(got) == set(range(9))  # every kind the ledger's passes can give; _GONE is the graph step's alone
    for r, k in zip(rows, got):  # a refused position is never a repeat, and whether a position is accepted does not depend on `earlier`
        first = got[rows.index(r[:6] + (0,))]
        assert k == (K.HQ_FAIL_REPEAT if r[6] and first in K.HQ_FAIL_ACCEPTED else first)


def test_the_rule_refuses_bad_arguments():
    lib = _debug_lib()
    z = np.zeros(1, np.uint8); bad = np.full(1, 3, np.uint8); p = lambda a: a.ctypes.data_as(abi.u8p)
    assert lib.hqtick_debug_fail_kind(1, p(z), p(bad), p(z), p(z), p(z), p(z), p(z), p(z)) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_fail_kind(1, None, p(z), p(z), p(z), p(z), p(z), p(z), p(z)) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_fail_kind(0, *([None] * 8)) == 0


# ---------------------------------------------------------------------------------------------- the mirror's lists
@pytest.mark.parametrize("name", sorted(fl.shapes()))
def test_shapes_on_the_mirror(name):
    """the lists of every shape are what one task_failed after the other gives: position i's list is the closure of its root among the tasks still here"""
    e, pairs = fl.shapes()[name]
    live = {x for x, t in e.tasks.items() if t.state != core.FINISHED}
    cons = {x: list(t.consumers) for x, t in e.tasks.items()}
    n = e.fail_tasks(pairs)
    assert n == sum(k in K.HQ_FAIL_ACCEPTED for k in e.last_fail_kinds)
    for (tid, wid), kind, mine in zip(pairs, e.last_fail_kinds, e.last_fail_consumers):
        if kind not in K.HQ_FAIL_ACCEPTED:
            assert mine == []
            continue
        assert tid in live
        closure, stack = set(), list(cons[tid])
        while stack:
            x = stack.pop()
            if x in live and x not in closure and x != tid:
                closure.add(x); stack.extend(cons[x])
        assert mine == sorted(closure)
        live -= closure | {tid}
    assert live == {x for x, t in e.tasks.items() if t.state != core.FINISHED}


def test_shapes_hold_what_they_are_for():
    s = fl.shapes()
    e, pairs = s["relabel_depth_2_vs_3"]
    d = {i: fl.depths_from(e, t) for i, (t, w) in enumerate(pairs)}
    e.fail_tasks(pairs)
    assert fl.owner_is_not_the_nearest(d, e.last_fail_kinds, e.last_fail_consumers)
    shared = [c for c in e.last_fail_consumers[0] if d[0][c] == 3 and d[1].get(c) == 2]
    assert len(shared) == 1  # reached at depth 2 from position 1, at depth 3 from position 0, owned by position 0
    e, pairs = s["waiting_root_gone"]
    e.fail_tasks(pairs)
    assert e.last_fail_kinds == [K.HQ_FAIL_WAITING, K.HQ_FAIL_ASSIGNED, K.HQ_FAIL_GONE, K.HQ_FAIL_ASSIGNED, K.HQ_FAIL_WAITING, K.HQ_FAIL_REPEAT, K.HQ_FAIL_NONE,
                                 K.HQ_FAIL_NOT_WAITING]
    assert pairs[2][0] in e.last_fail_consumers[1] and e.last_fail_consumers[3] == []
    e, pairs = s["chain_of_70"]
    e.fail_tasks(pairs)
    assert [len(c) for c in e.last_fail_consumers] == [35, 0, 35]
    e, pairs = s["fan_of_300"]
    e.fail_tasks(pairs)
    assert [len(c) for c in e.last_fail_consumers] == [100, 200]


# ---------------------------------------------------------------------------------------------- what the GPU suite's histories contain
def test_histories_meet_every_kind_and_a_far_owner():
    """a GPU test that never meets a kind would hide that kind: across their seeds the histories of tests/test_gpu_fail.py give every one of the ten kinds, at least
    one consumer whose owner is not the root that reaches it in the fewest steps, and never more than one Retracting id in four failed ones"""
    seen = collections.Counter()
    far = 0
    for seed in fl.HISTORY_SEEDS:
        e, pairs = fl.history(seed)
        depth = {i: fl.depths_from(e, t) if t in e.tasks else {} for i, (t, w) in enumerate(pairs)}
        n = e.fail_tasks(pairs)
        kinds = e.last_fail_kinds
        seen.update(kinds)
        far += fl.owner_is_not_the_nearest(depth, kinds, e.last_fail_consumers)
        assert n >= 4 and 4 * sum(k == K.HQ_FAIL_RETRACTING for k in kinds) <= n
        assert all(t.state == core.WAITING for t in e.tasks.values() if t.state != core.FINISHED and t.unfinished_deps) # what is left is a valid state
    assert set(seen) == set(range(10)), sorted(seen.items())
    assert far >= 1


# ---------------------------------------------------------------------------------------------- the new symbols
def test_new_symbols_in_headers_libraries_and_bindings():
    build.build()
    hdr = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    dbg = open(os.path.join(ROOT, "include", "hqtick_debug.h")).read()
    rs = open(os.path.join(ROOT, "integration", "hqtick_sys.rs")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr) and re.search(r"pub fn %s\(" % name, rs)
    for k, name in enumerate(NAMES):
        assert re.search(r"#define HQ_FAIL_%s\s+%d\b" % (name, k), hdr) and "pub const HQ_FAIL_%s: u32 = %d;" % (name, k) in rs
    assert "hqtick_debug_fail_kind(" in dbg and "hqtick_debug_fail_kind" not in hdr
    prod = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    test = subprocess.run(["nm", "-D", "--defined-only", build.TEST_LIB], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\b" % name, prod) and re.search(r"\b%s\b" % name, test)
    assert "hqtick_debug_fail_kind" in test and "hqtick_debug_fail_kind" not in prod  # the hook is the test library's alone
    assert abi.HQTICK_ABI_VERSION == 12  # added within ABI 12: no struct changed
