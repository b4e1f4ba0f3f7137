"""SchedEnv.reject_tasks, the mirror's task_reject / request_enabled (server/reactor.rs:365-460): the scenarios of tests/reject_cases.py with the reference's
outcomes, the decision rule of hqtick_reject_tasks (csrc/reject_core.h through hqtick_debug_reject_kind) over the full table of its inputs against a restatement
written here, the call's bad arguments, the new symbols in headers, libraries and bindings, and the seeded histories on the mirror with the coverage conditions
that keep the GPU run from passing on empty ground.  The CPU oracle is the scheduler.  No GPU needed."""
import collections
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
import reject_cases as rj
from hyperqueue_amd import abi, build, core, tick
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hqtick_reject_tasks", "hqtick_reject_last_routes", "hqtick_reject_last_requeued", "hqtick_reject_last_reassigned", "hqtick_cluster_enable_request", "hqtick_cluster_blocked"]
KINDS = {"HQ_REJECT_NONE": 0, "HQ_REJECT_ASSIGNED": 1, "HQ_REJECT_PREFILLED": 2, "HQ_REJECT_RETRACTING": 3, "HQ_REJECT_REDIRECTED": 4, "HQ_REJECT_REPEAT": 5,
         "HQ_REJECT_WRONG_WORKER": 6, "HQ_REJECT_WRONG_VARIANT": 7, "HQ_REJECT_RUNNING": 8, "HQ_REJECT_BAD_VARIANT": 9, "HQ_REJECT_MN": 10}
K = abi
SN, MN, PF = 0, 1, 2
N_IN = 12  # input columns of hqtick_debug_reject_kind


@pytest.fixture(scope="module")
def backend():
    return Oracle(abi.make_config(reserve=1, fill_max=1, time_limit_s=20.0))


def _debug_lib():
    build.build()
    lib = C.CDLL(build.TEST_LIB)
    lib.hqtick_debug_reject_kind.argtypes = [C.c_uint32] + [abi.u8p] * (N_IN + 2)
    lib.hqtick_debug_reject_kind.restype = C.c_int
    return lib


def _rule(lib, rows):
    cols = [np.ascontiguousarray([r[k] for r in rows], np.uint8) for k in range(N_IN)]
    kind = np.full(len(rows), 255, np.uint8); blocks = np.full(len(rows), 255, np.uint8)
    assert lib.hqtick_debug_reject_kind(len(rows), *[c.ctypes.data_as(abi.u8p) for c in cols], kind.ctypes.data_as(abi.u8p), blocks.ctypes.data_as(abi.u8p)) == len(rows)
    return kind.tolist(), blocks.tolist()


# The rule's table (the issue's), one line per state of the id before the batch: (what must hold of the inputs, the kind).  The first line that matches
# decides; None: the input is not read.  Inputs: entry found, class, entry worker == reporter, entry variant == rejected, running byte, no variant named, the request
# has the variant, override found, override's FROM worker == reporter, the override holds a redirect.  A named variant the request lacks is "bad".
def _bad(vn, vx):
    return not vn and not vx


TABLE = [
    # found cls   wm    vm    run   of  om    red
    ((None, None, None, None, None, 1,  1,    1), False, K.HQ_REJECT_REDIRECTED),
    ((None, None, None, None, None, 1,  1,    0), False, K.HQ_REJECT_RETRACTING),
    ((None, None, None, None, None, 1,  1,    None), True, K.HQ_REJECT_BAD_VARIANT),
    ((None, None, None, None, None, 1,  0,    None), None, K.HQ_REJECT_WRONG_WORKER),
    ((0,    None, None, None, None, 0,  None, None), None, K.HQ_REJECT_NONE),
    ((1,    MN,   None, None, None, 0,  None, None), None, K.HQ_REJECT_MN),
    ((1,    None, 0,    None, None, 0,  None, None), None, K.HQ_REJECT_WRONG_WORKER),
    ((1,    None, 1,    None, None, 0,  None, None), True, K.HQ_REJECT_BAD_VARIANT),
    ((1,    PF,   1,    None, None, 0,  None, None), False, K.HQ_REJECT_PREFILLED),
    ((1,    SN,   1,    None, 1,    0,  None, None), False, K.HQ_REJECT_RUNNING),
    ((1,    SN,   1,    1,    0,    0,  None, None), False, K.HQ_REJECT_ASSIGNED),   # (with a variant named: see _restated)
    ((1,    SN,   1,    None, 0,    0,  None, None), False, K.HQ_REJECT_WRONG_VARIANT),
]
ACCEPTED = (K.HQ_REJECT_ASSIGNED, K.HQ_REJECT_PREFILLED, K.HQ_REJECT_RETRACTING, K.HQ_REJECT_REDIRECTED)
BLOCKS = ACCEPTED + (K.HQ_REJECT_WRONG_WORKER, K.HQ_REJECT_WRONG_VARIANT)


def _restated(row):
    f, c, wm, vm, run, vn, vx, of, om, red, earlier, resident = row
    inputs = (f, c, wm, vm, run, of, om, red)
    for want, bad, kind in TABLE:
        if not all(w is None or w == x for w, x in zip(want, inputs)):
            continue
        if bad is not None and bad != _bad(vn, vx):
            continue
        if kind == K.HQ_REJECT_ASSIGNED and vn:  # None is never the entry's variant (resource_rq_variant != Some(*rv_id))
            continue
        kind = K.HQ_REJECT_REPEAT if earlier and kind in ACCEPTED else kind
        return kind, int(kind in BLOCKS and not vn and vx and resident)
    raise AssertionError(row)


# ---------------------------------------------------------------------------------------------- the rule
def test_the_rule_over_its_full_table():
    lib = _debug_lib()
    assert [getattr(abi, k) for k in KINDS] == list(KINDS.values()) == list(range(11))
    assert set(abi.HQ_REJECT_ACCEPTED) == set(abi.HQ_REJECT_ELIGIBLE) == set(ACCEPTED) and set(abi.HQ_REJECT_BLOCKS) == set(BLOCKS)
    assert set(abi.HQ_REJECT_SCHEDULES) == set(ACCEPTED) - {K.HQ_REJECT_REDIRECTED}
    rows = [(f, c) + rest for f in (0, 1) for c in (SN, MN, PF) for rest in itertools.product((0, 1), repeat=10)]
    assert len(rows) == 6144 and len(set(rows)) == 6144
    kinds, blocks = _rule(lib, rows)
    want = [_restated(r) for r in rows]
    assert kinds == [w[0] for w in want]
    assert blocks == [w[1] for w in want]
    assert set(kinds) == set(range(11))  # every kind occurs
    by_kind = collections.defaultdict(set)
    for k, b in zip(kinds, blocks):
        by_kind[k].add(b)
    for k in range(11):  # the kinds that change nothing at all never block; the others do exactly when the pair can be named
        assert by_kind[k] == ({0, 1} if k in BLOCKS else {0}), k
    for r, k in zip(rows, kinds):  # a refused kind never becomes a repeat
        if r[10]:
            first = kinds[rows.index(r[:10] + (0,) + r[11:])]
            assert k == (K.HQ_REJECT_REPEAT if first in ACCEPTED else first)


def test_the_rule_refuses_bad_arguments():
    lib = _debug_lib()
    z = np.zeros(1, np.uint8); bad = np.full(1, 3, np.uint8); p = lambda a: a.ctypes.data_as(abi.u8p)
    assert lib.hqtick_debug_reject_kind(1, p(z), p(bad), *([p(z)] * (N_IN - 2)), p(z), p(z)) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_reject_kind(1, None, *([p(z)] * (N_IN + 1))) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_reject_kind(1, *([p(z)] * N_IN), None, p(z)) == abi.HQTICK_E_INVALID
    out = np.full(1, 255, np.uint8)
    assert lib.hqtick_debug_reject_kind(1, *([p(z)] * N_IN), p(out), None) == 1 and out.tolist() == [K.HQ_REJECT_NONE]  # (the blocks column is optional)
    assert lib.hqtick_debug_reject_kind(0, *([None] * (N_IN + 2))) == 0


# ---------------------------------------------------------------------------------------------- the reference's scenarios on the mirror
def _env(backend_cfg=None):
    cfg = abi.make_config(time_limit_s=20.0, **(backend_cfg or {}))
    e = SchedEnv(cfg)
    return e, rj.MirrorSide(e, Oracle(cfg))


def test_task_reject1():
    e, side = _env()
    w, t = rj.setup_reject1(e)
    side.schedule()
    rj.act_reject1(side, e, w, t)


def test_task_reject2():
    e, side = _env()
    w, t = rj.setup_reject2(e)
    side.schedule()
    rj.act_reject2(side, e, w, t)
    assert e.workers[w].blocked_requests == {(e.tasks[t].rq, 0)}


def test_task_reject3():
    e, side = _env()
    w, t1, t2 = rj.setup_reject3(e)
    side.schedule()
    rj.act_reject3(side, e, w, t1, t2)
    assert e.workers[w].blocked_requests == {(e.tasks[t1].rq, 0)}  # a pair already blocked is not added twice


def test_prefill_rejected(backend):
    e, w1, tasks, assigned, prefilled = cc.setup_prefill(backend)
    rj.act_prefill_rejected(rj.MirrorSide(e, backend), e, w1, prefilled)
    assert e.task(assigned).is_assigned()
    # any variant, None included, takes a prefilled task back; None blocks nothing
    e, w1, tasks, assigned, prefilled = cc.setup_prefill(backend)
    assert e.reject_tasks([(prefilled, w1, None)]) == 1 and e.last_reject_kinds == [K.HQ_REJECT_PREFILLED]
    assert e.tasks[prefilled].state == core.WAITING and not e.workers[w1].blocked_requests


def test_steal_rejected(backend):
    e, w1, w2, t, on_w1 = fc.scenario_steal(backend)
    free_w2 = list(e.workers[w2].free)
    rj.act_steal_rejected(rj.MirrorSide(e, backend), e, w1, w2, t)
    assert e.workers[w2].free == free_w2  # the target's entry stays: nothing is released


def test_the_refusals_change_nothing_and_the_blocks_follow_the_kind(backend):
    e, w1, w2, t, on_w1 = fc.scenario_steal(backend)
    (on_w2,) = [x for x in e.workers[w2].assigned_tasks if x != t]
    e.start_tasks([(on_w2, w2, e.tasks[on_w2].rv)])
    rq = e.tasks[t].rq
    batch = [(t, w2, 0), (on_w1, w2, 0), (on_w1, w1, None), (on_w1, w1, 5), (on_w2, w2, 0), (10**12, w1, 0), (on_w1, rj.GHOST, 0), (on_w1, w1, 0), (on_w1, w1, 0), (t, w1, 7)]
    assert e.reject_tasks(batch) == 1
    assert e.last_reject_kinds == [K.HQ_REJECT_WRONG_WORKER, K.HQ_REJECT_WRONG_WORKER, K.HQ_REJECT_WRONG_VARIANT, K.HQ_REJECT_BAD_VARIANT, K.HQ_REJECT_RUNNING, K.HQ_REJECT_NONE,
                                   K.HQ_REJECT_WRONG_WORKER, K.HQ_REJECT_ASSIGNED, K.HQ_REJECT_REPEAT, K.HQ_REJECT_BAD_VARIANT]
    # w2 blocked the pair twice (once is kept), w1 once; None, a bad variant, a running task, an unknown id, a ghost worker and a repeat block nothing
    assert e.workers[w2].blocked_requests == {(rq, 0)} and e.workers[w1].blocked_requests == {(rq, 0)}
    assert e.tasks[t].state == core.RETRACTING and t in e.redirects and e.tasks[on_w2].state == core.RUNNING
    assert e.last_reject_requeued == [(on_w1, rq, e.tasks[on_w1].priority)]


def test_a_retracting_task_without_a_redirect_is_not_added_twice():
    e = SchedEnv()
    w = e.new_worker_cpus(2)
    t = e.new_task()
    x = e.tasks[t]; x.state, x.worker = core.RETRACTING, w  # as process_retracted leaves it: Retracting{w}, in its queue
    assert t in e.ready[x.rq]
    assert e.reject_tasks([(t, w, 0), (t, w, 0)]) == 1 and e.last_reject_kinds == [K.HQ_REJECT_RETRACTING, K.HQ_REJECT_REPEAT]
    assert x.state == core.WAITING and x.worker is None and e.last_reject_requeued == [] and sum(len(s) for s in e.ready.values()) == 1


def _prefill_under_a_high_priority_task(backend):
    """a full 1-cpu worker that holds a task of user priority 5 (assigned by hand), then test_reactor.rs:775-795's three tasks and 1-cpu worker and one tick
    -> (mirror, the high task, its worker, the prefilled tasks as (worker, task))"""
    e = SchedEnv(abi.make_config(reserve=1, fill_max=1, time_limit_s=20.0))
    w2 = e.new_worker(WB(1))
    hi = e.new_task(TB().user_priority(5))
    e.assign_task(hi, w2)
    e.new_tasks(3, TB())
    e.new_worker(WB(1))
    e.schedule(backend)
    pf = sorted((t.worker, x) for x, t in e.tasks.items() if t.state == core.PREFILLED)
    assert pf
    return e, hi, w2, pf


def test_a_requeued_task_dissolves_the_lower_prefill_sets_after_the_batch(backend):
    e, hi, w2, pf = _prefill_under_a_high_priority_task(backend)
    mark = len(e.retract_messages)
    assert e.reject_tasks([(hi, w2, 0)]) == 1
    assert sorted(e.retract_messages[mark:]) == pf
    for (_, x) in pf:
        assert e.tasks[x].state == core.RETRACTING and x in e.ready[e.tasks[x].rq]
    # ... and a prefilled task of that set rejected in the same batch, behind the arrival, is taken as Prefilled: it waits in its queue either way
    e, hi, w2, pf = _prefill_under_a_high_priority_task(backend)
    (w, x) = pf[0]
    mark = len(e.retract_messages)
    assert e.reject_tasks([(hi, w2, 0), (x, w, 0)]) == 2 and e.last_reject_kinds == [K.HQ_REJECT_ASSIGNED, K.HQ_REJECT_PREFILLED]
    assert sorted(e.retract_messages[mark:]) == pf[1:] and e.tasks[x].state == core.WAITING and [y[0] for y in e.last_reject_requeued] == sorted([hi, x])


# ---------------------------------------------------------------------------------------------- the histories on the mirror
def _played(form):
    out = []
    for seed in rj.SEEDS[form]:
        oracle = Oracle(abi.make_config(reserve=1, fill_max=2, **rj.lc.CFG), canonical=True)
        out.append(rj.play(rj.history(seed, form), oracle))
    return out


def test_histories_cover_the_ground_on_the_mirror_alone():
    cov = {}
    for form in rj.FORMS:
        hs = _played(form)
        c = collections.Counter()
        for h in hs:
            c.update(h.cov)
            assert h.rounds_done >= 3, (form, h.seed, h.rounds_done)
        cov[form] = c
        for k in ACCEPTED + (K.HQ_REJECT_REPEAT, K.HQ_REJECT_WRONG_WORKER, K.HQ_REJECT_WRONG_VARIANT, K.HQ_REJECT_NONE, K.HQ_REJECT_RUNNING):
            assert c[f"HQ_REJECT_{k}"] > 0, (form, k)
        assert c["reject dissolved a prefill set"] > 0, form
        assert c["tick placed an enabled request"] > 0, form
    lines = rj.coverage_lines(cov)
    path = os.path.join(ROOT, "profiles", "reject", "coverage.txt")
    text = "kinds and events of the reject histories (tests/reject_cases.py SEEDS) on the mirror, per form\n" + "\n".join(lines) + "\n"
    print(text)
    if not os.path.exists(path):  # (the table is written once and committed; from then on it is compared: delete the file to write it anew)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "w").write(text)
    assert open(path).read() == text


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
    assert re.search(r"\bint hqtick_debug_reject_kind\(", d)
    assert "hqtick_debug_reject_kind" not in h
    m = open(os.path.join(ROOT, "hyperqueue_amd", "csrc", "exports.map")).read()
    assert "hqtick_*" in m  # (the map exports the C ABI by prefix: the new names need no line of their own)


def test_libraries_export_the_new_symbols():
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\s(hqtick_\w+)$", out, flags=re.M))
    for n in NEW:
        assert n in syms, n
    assert "hqtick_debug_reject_kind" not in syms  # the hook lives in the test library only
    out = subprocess.run(["nm", "-D", "--defined-only", build.TEST_LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\shqtick_debug_reject_kind$", out, flags=re.M)
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


def test_python_bindings_exist_and_bad_arguments_are_refused():
    for f in ("reject_tasks", "reject_last", "cluster_enable_request", "cluster_blocked"):
        assert callable(getattr(tick.Tick, f)), f
    assert callable(core.SchedEnv.reject_tasks)
    lib = tick.load()
    lib.hqtick_reject_tasks.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u8p, abi.u32p]
    lib.hqtick_reject_last_routes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u8p)]
    lib.hqtick_reject_last_requeued.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u64p)]
    lib.hqtick_reject_last_reassigned.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u64p), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
    lib.hqtick_cluster_enable_request.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint8]
    lib.hqtick_cluster_blocked.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
    ids = (C.c_uint64 * 2)(1, 2); ws = (C.c_uint32 * 2)(1, 1); vs = (C.c_uint8 * 2)(0, 0xFF)
    assert lib.hqtick_reject_tasks(None, 0, None, None, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_reject_tasks(None, 2, ids, ws, vs, None) == abi.HQTICK_E_INVALID
    n = C.c_uint32(7); k = abi.u8p()
    assert lib.hqtick_reject_last_routes(None, C.byref(n), C.byref(k)) == abi.HQTICK_E_INVALID
    assert n.value == 0 and not k
    assert lib.hqtick_reject_last_routes(None, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_reject_last_requeued(None, None, None, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_reject_last_reassigned(None, None, None, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_cluster_enable_request(None, 1, 0, 0) == abi.HQTICK_E_INVALID
    assert lib.hqtick_cluster_blocked(None, 1, None, None, None) == abi.HQTICK_E_INVALID
