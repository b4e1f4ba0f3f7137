"""SchedEnv.finish_tasks and SchedEnv.start_retracting_task, the mirror's task_finished (server/reactor.rs:510-590) and task_running's Retracting arm (:311-335):
the scenarios of tests/finish_cases.py with the reference's outcomes, the decision rule of hqtick_finish_tasks (csrc/finish_core.h through
hqtick_debug_finish_kind) against a table written out here, and the new symbols in headers, libraries and bindings.  The CPU oracle is the scheduler where a
scenario needs a tick.  No GPU needed."""
import ctypes as C
import importlib.util
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import cancel_cases as cc
import finish_cases as fc
from hyperqueue_amd import abi, build, core, tick
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB
from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hqtick_finish_tasks", "hqtick_finish_last_routes", "hqtick_retracting_started"]
KINDS = {"HQ_FINISH_NONE": 0, "HQ_FINISH_ASSIGNED": 1, "HQ_FINISH_MN": 2, "HQ_FINISH_RETRACTING": 3, "HQ_FINISH_REPEAT": 4, "HQ_FINISH_WRONG_WORKER": 5,
         "HQ_FINISH_PREFILLED": 6}
N, A, M, T, R, W, P = range(7)  # NONE, ASSIGNED, MN, RETRACTING, REPEAT, WRONG_WORKER, PREFILLED

# The rule, written out.  Rows: (entry found, entry class 0 single-node / 1 multi-node / 2 prefilled, entry worker == reporter).  Columns: (override found,
# override worker == reporter, an earlier position was accepted) = 000 001 010 011 100 101 110 111.  An id of the Retracting table is decided by the table alone
# (columns 100..111 are the same in every row); without an override the override's worker is not read (columns 010, 011 repeat 000, 001); without an entry its
# class and worker are not read (the first six rows are one).
RULE = {
    (0, 0, 0): (N, N, N, N, W, W, T, R),
    (0, 0, 1): (N, N, N, N, W, W, T, R),
    (0, 1, 0): (N, N, N, N, W, W, T, R),
    (0, 1, 1): (N, N, N, N, W, W, T, R),
    (0, 2, 0): (N, N, N, N, W, W, T, R),
    (0, 2, 1): (N, N, N, N, W, W, T, R),
    (1, 0, 0): (W, W, W, W, W, W, T, R),
    (1, 0, 1): (A, R, A, R, W, W, T, R),
    (1, 1, 0): (W, W, W, W, W, W, T, R),
    (1, 1, 1): (M, R, M, R, W, W, T, R),
    (1, 2, 0): (P, P, P, P, W, W, T, R),
    (1, 2, 1): (P, P, P, P, W, W, T, R),
}


@pytest.fixture(scope="module")
def backend():
    return Oracle(abi.make_config(reserve=1, fill_max=1, time_limit_s=20.0))


def _debug_lib():
    build.build()
    lib = C.CDLL(build.TEST_LIB)
    lib.hqtick_debug_finish_kind.argtypes = [C.c_uint32] + [abi.u8p] * 7
    lib.hqtick_debug_finish_kind.restype = C.c_int
    return lib


def _rule(lib, rows):
    cols = [np.ascontiguousarray([r[k] for r in rows], np.uint8) for k in range(6)]
    out = np.full(len(rows), 255, np.uint8)
    assert lib.hqtick_debug_finish_kind(len(rows), *[c.ctypes.data_as(abi.u8p) for c in cols], out.ctypes.data_as(abi.u8p)) == len(rows)
    return out.tolist()


# ---------------------------------------------------------------------------------------------- the rule
def test_the_rule_against_the_written_table():
    lib = _debug_lib()
    assert [KINDS[k] for k in ("HQ_FINISH_NONE", "HQ_FINISH_ASSIGNED", "HQ_FINISH_MN", "HQ_FINISH_RETRACTING", "HQ_FINISH_REPEAT", "HQ_FINISH_WRONG_WORKER", "HQ_FINISH_PREFILLED")] == [N, A, M, T, R, W, P]
    rows, want = [], []
    for (found, cls, wm), line in RULE.items():
        for col, (of, om, earlier) in enumerate(itertools.product((0, 1), repeat=3)):
            rows.append((found, cls, wm, of, om, earlier)); want.append(line[col])
    assert len(rows) == 96 and len(set(rows)) == 96  # every combination of the six inputs, the class three-valued: the 2^6 of two classes and the third's 32
    assert _rule(lib, rows) == want
    # what is accepted never depends on `earlier`, and `earlier` turns exactly the accepted kinds into a repeat
    for r, k in zip(rows, want):
        if r[5]:
            first = want[rows.index(r[:5] + (0,))]
            assert k == (R if first in abi.HQ_FINISH_ACCEPTED else first)


def test_the_rule_refuses_bad_arguments():
    lib = _debug_lib()
    z = np.zeros(1, np.uint8); bad = np.full(1, 3, np.uint8); p = lambda a: a.ctypes.data_as(abi.u8p)
    assert lib.hqtick_debug_finish_kind(1, p(z), p(bad), p(z), p(z), p(z), p(z), p(z)) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_finish_kind(1, None, p(z), p(z), p(z), p(z), p(z), p(z)) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_finish_kind(0, None, None, None, None, None, None, None) == 0


def _rule_inputs(e: SchedEnv, tid, wid, accepted_by):
    """the six inputs of the rule as a ledger + Retracting-table host would see them for (tid, wid), from the mirror BEFORE the pair is applied"""
    t = e.tasks.get(tid)
    if tid in accepted_by:
        t_state, t_worker, t_target = accepted_by[tid]
    elif t is None:
        t_state, t_worker, t_target = None, None, None
    else:
        t_target = e.redirects[tid][0] if tid in e.redirects else (t.worker if tid in e.retaken_variant else None)
        t_state, t_worker = t.state, (t.mn_workers[0] if t.state == core.RUNNING_MN else t.worker)
    of = t_state == core.RETRACTING
    if of:  # the ledger's entry, if any, is the redirect target's (or the old worker's own, retaken)
        found, cls, wm = t_target is not None, 0, t_target == wid
    else:
        found = t_state in (core.ASSIGNED, core.RUNNING, core.RUNNING_MN, core.PREFILLED)
        cls = {core.RUNNING_MN: 1, core.PREFILLED: 2}.get(t_state, 0)
        wm = found and t_worker == wid
    return (int(found), cls, int(bool(wm)), int(of), int(of and t_worker == wid), 0), (t_state, t_worker, t_target)


def _kinds_by_rule(lib, e: SchedEnv, pairs):
    """what the rule says for the batch, evaluated position by position on a copy of the mirror's view (an accepted position is remembered as it was: every
    position of the device's batch sees the tables as they were BEFORE the batch)"""
    accepted_by, kinds = {}, []
    for tid, wid in pairs:
        inputs, seen = _rule_inputs(e, tid, wid, accepted_by)
        first = _rule(lib, [inputs])[0]
        earlier = tid in accepted_by
        k = _rule(lib, [inputs[:5] + (int(earlier),)])[0]
        kinds.append(k)
        if first in abi.HQ_FINISH_ACCEPTED and not earlier:
            accepted_by[tid] = seen
    return kinds


# ---------------------------------------------------------------------------------------------- the scenarios on the mirror
def test_assignments_and_finish():
    lib = _debug_lib()
    e, ws, steps, t = fc.scenario_assignments_and_finish()
    for pairs, held, released in steps:
        by_rule = _kinds_by_rule(lib, e, pairs)
        assert e.finish_tasks(pairs) == released
        assert e.last_finish_kinds == [abi.HQ_FINISH_ASSIGNED] == by_rule  # one accepted position: need_scheduling
        assert e.tasks[pairs[0][0]].state == core.FINISHED
        assert {w: set(e.workers[w].assigned_tasks) for w in ws} == held
    assert all(w.free == w.total for w in e.workers.values())
    assert t["t3"] in e.ready[e.tasks[t["t3"]].rq] and e.tasks[t["t7"]].unfinished_deps == 1


def test_mn_finish_by_its_root():
    lib = _debug_lib()
    e, t1, root, other = fc.scenario_mn_finish()
    pairs = [(t1, other), (t1, root), (t1, root), (t1, other)]
    by_rule = _kinds_by_rule(lib, e, pairs)
    assert e.finish_tasks(pairs) == []
    assert e.last_finish_kinds == [abi.HQ_FINISH_WRONG_WORKER, abi.HQ_FINISH_MN, abi.HQ_FINISH_REPEAT, abi.HQ_FINISH_WRONG_WORKER] == by_rule
    assert all(w.mn_task is None and w.sn() and w.free == w.total for w in e.workers.values())
    assert e.tasks[t1].state == core.FINISHED


def test_steal_finished(backend):
    lib = _debug_lib()
    e, w1, w2, t, on_w1 = fc.scenario_steal(backend)
    before = e.workers[w2].free[0]
    assert e.finish_tasks([(t, w2)]) == [] and e.last_finish_kinds == [abi.HQ_FINISH_WRONG_WORKER]  # the redirect TARGET never got the task
    assert e.tasks[t].state == core.RETRACTING and e.workers[w2].free[0] == before
    assert _kinds_by_rule(lib, e, [(t, w2), (t, w1)]) == [abi.HQ_FINISH_WRONG_WORKER, abi.HQ_FINISH_RETRACTING]
    assert e.finish_tasks([(t, w1)]) == []
    fc.check_steal_finished(e, w1, w2, t, before)
    e.retract_response(w1, [t])  # the worker's late answer finds no such task
    assert e.tasks[t].state == core.FINISHED


def test_steal_running(backend):
    e, w1, w2, t, on_w1 = fc.scenario_steal(backend)
    assert e.finish_tasks([(on_w1, w1)]) == [] and e.last_finish_kinds == [abi.HQ_FINISH_ASSIGNED]
    assert not e.start_retracting_task(t, w2) and e.tasks[t].state == core.RETRACTING  # not the worker it is retracting from
    assert e.start_retracting_task(t, w1, 0)
    fc.check_steal_running(e, w1, w2, t, on_w1)
    assert not e.start_retracting_task(t, w1, 0)  # Running now


def test_retracting_in_its_queue_and_refusals(backend):
    """a prefill set dissolved by a higher-priority arrival: its task is Retracting in its queue, no redirect.  Finished by its worker it leaves the queue (the
    library's reading); a prefilled, a waiting and an unknown id are refused and change nothing"""
    lib = _debug_lib()
    e, w1, tasks, assigned, prefilled = cc.setup_prefill(backend)
    waiting = next(x for x in tasks if x not in (assigned, prefilled))
    pairs = [(prefilled, w1), (waiting, w1), (10**9, w1)]
    assert _kinds_by_rule(lib, e, pairs) == [abi.HQ_FINISH_PREFILLED, abi.HQ_FINISH_NONE, abi.HQ_FINISH_NONE]
    free = list(e.workers[w1].free)
    assert e.finish_tasks(pairs) == [] and e.last_finish_kinds == [abi.HQ_FINISH_PREFILLED, abi.HQ_FINISH_NONE, abi.HQ_FINISH_NONE]
    assert e.tasks[prefilled].state == core.PREFILLED and e.tasks[waiting].state == core.WAITING and e.workers[w1].free == free
    e.new_task(TB().cpus(1).user_priority(10))
    assert e.tasks[prefilled].is_retracting() and prefilled in e.ready[e.tasks[prefilled].rq]
    pairs = [(prefilled, w1 + 1), (prefilled, w1), (prefilled, w1)]
    by_rule = _kinds_by_rule(lib, e, pairs)
    assert e.finish_tasks(pairs) == []
    assert e.last_finish_kinds == [abi.HQ_FINISH_WRONG_WORKER, abi.HQ_FINISH_RETRACTING, abi.HQ_FINISH_REPEAT] == by_rule
    assert all(prefilled not in s for s in e.ready.values()) and e.workers[w1].free == free


def test_the_last_all_order_rule_with_a_refused_position_between():
    rows = []
    for first_all in (False, True):
        e = SchedEnv()
        w, w_other = e.new_workers_cpus([4, 4])
        a = e.new_task(TB().cpus(1)); b = e.new_task(TB().cpus_all())
        e.assign_task(a, w); e.assign_task(b, w)
        x, y = (b, a) if first_all else (a, b)
        e.finish_tasks([(x, w), (y, w_other), (y, w)])
        assert e.last_finish_kinds == [abi.HQ_FINISH_ASSIGNED, abi.HQ_FINISH_WRONG_WORKER, abi.HQ_FINISH_ASSIGNED]
        rows.append(list(e.worker(w).free))
    assert rows[0] == e.worker(w).total and rows[1][0] == rows[0][0] + core.amount(1)


def test_consumers_are_released_once_and_not_by_refused_producers():
    e = SchedEnv()
    ws = e.new_workers_cpus([4, 4])
    a = e.new_task(TB().cpus(1)); b = e.new_task(TB().cpus(1)); r = e.new_task(TB().cpus(1))
    both = e.new_task(TB().cpus(1).task_deps([a, b])); of_r = e.new_task(TB().cpus(1).task_deps([r]))
    e.assign_task(a, ws[0]); e.assign_task(b, ws[1]); e.assign_task(r, ws[1])
    assert e.finish_tasks([(a, ws[0]), (r, ws[0]), (b, ws[1]), (a, ws[0])]) == [both]
    assert e.last_finish_kinds == [abi.HQ_FINISH_ASSIGNED, abi.HQ_FINISH_WRONG_WORKER, abi.HQ_FINISH_ASSIGNED, abi.HQ_FINISH_REPEAT]
    assert e.tasks[of_r].unfinished_deps == 1 and e.tasks[r].state == core.ASSIGNED


# ---------------------------------------------------------------------------------------------- headers, libraries, bindings
def test_prototypes_are_declared_and_the_version_stays_12():
    h = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\((const )?hqtick_ctx \*ctx", h), n
    assert "#define HQTICK_ABI_VERSION 12u" in h and abi.HQTICK_ABI_VERSION == 12
    for name, value in KINDS.items():
        assert re.search(r"#define " + name + r"\s+" + str(value) + r"\b", h), name
        assert getattr(abi, name) == value
    d = open(os.path.join(ROOT, "include", "hqtick_debug.h")).read()
    assert re.search(r"\bint hqtick_debug_finish_kind\(", d)


def test_libraries_export_the_new_symbols():
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\s(hqtick_\w+)$", out, flags=re.M))
    for n in NEW:
        assert n in syms, n
    h = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    for s in syms:
        if s.startswith("hqtick_finish") or s.startswith("hqtick_retracting"):
            assert re.search(r"\b" + s + r"\(", h), s  # absent from no header
    assert "hqtick_debug_finish_kind" not in syms  # the hook lives in the test library only
    out = subprocess.run(["nm", "-D", "--defined-only", build.TEST_LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\shqtick_debug_finish_kind$", out, flags=re.M)
    for n in NEW:
        assert re.search(r"\s" + n + r"$", out, flags=re.M), n


def test_rust_binding_is_regenerated():
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "tools", "gen_rust_sys.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    text = open(os.path.join(ROOT, "integration", "hqtick_sys.rs")).read()
    assert text == gen.generate()
    for n in NEW:
        assert re.search(r"pub fn " + n + r"\(", text), n
    for name in KINDS:
        assert name in text, name


def test_python_bindings_exist_and_a_null_context_is_refused():
    assert callable(tick.Tick.finish_tasks) and callable(tick.Tick.retracting_started)
    assert callable(core.SchedEnv.finish_tasks) and callable(core.SchedEnv.start_retracting_task)
    lib = tick.load()
    lib.hqtick_finish_tasks.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p]
    lib.hqtick_finish_last_routes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u8p)]
    lib.hqtick_retracting_started.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u32p, abi.u8p, abi.u64p]
    ids = (C.c_uint64 * 2)(1, 2); ws = (C.c_uint32 * 2)(1, 1)
    assert lib.hqtick_finish_tasks(None, 0, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_finish_tasks(None, 2, ids, ws) == abi.HQTICK_E_INVALID
    n = C.c_uint32(7); k = abi.u8p()
    assert lib.hqtick_finish_last_routes(None, C.byref(n), C.byref(k)) == abi.HQTICK_E_INVALID
    assert n.value == 0 and not k
    assert lib.hqtick_finish_last_routes(None, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_retracting_started(None, 0, None, None, None, None, None) == abi.HQTICK_E_INVALID
