"""SchedEnv.lose_workers, the mirror's on_remove_worker for a batch (server/reactor.rs:64-186): on every lifecycle history a batch of one worker is remove_worker
exactly; the rule of hqtick_lose_workers (csrc/lose_core.h through hqtick_debug_lose_kind) over the full table of its inputs against a restatement written here;
the grouping's phases (hqtick_debug_lose_group) against a numpy stable argsort at the wavefront, tile and padding edges; the batched histories of
tests/lose_cases.py on the mirror with the coverage lines that keep the GPU run from passing on empty ground; the new symbols in headers, libraries and
bindings.  The CPU oracle is the scheduler.  No GPU needed."""
import collections
import copy
import ctypes as C
import importlib.util
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import lifecycle_cases as lc
import lose_cases as ls
from hyperqueue_amd import abi, build, core, tick
from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hqtick_lose_workers", "hqtick_lose_last_tasks", "hqtick_lose_last_requeued", "hqtick_lose_last_reassigned", "hqtick_lose_last_mn_left"]
KINDS = {"HQ_LOSE_ASSIGNED": 0, "HQ_LOSE_RUNNING": 1, "HQ_LOSE_PREFILLED": 2, "HQ_LOSE_MN_ROOT": 3, "HQ_LOSE_REDIRECT": 4}
K = abi
SN, MN, PF = 0, 1, 2


def _debug_lib():
    build.build()
    lib = C.CDLL(build.TEST_LIB)
    lib.hqtick_debug_lose_kind.argtypes = [C.c_uint32] + [abi.u8p] * 5
    lib.hqtick_debug_lose_kind.restype = C.c_int
    lib.hqtick_debug_lose_group.argtypes = [C.c_uint32, C.c_uint32, abi.u64p, abi.u64p, abi.u32p, abi.u8p, abi.u32p, C.c_int, abi.u32p, abi.u64p, abi.u64p, abi.u32p, abi.u8p]
    lib.hqtick_debug_lose_group.restype = C.c_int
    return lib


# ---------------------------------------------------------------------------------------------- the rule
def _restated(cls, run, redirect):
    """the issue's table: the entry's variant class and running byte decide; a single-node entry on a Retracting task's redirect target is the redirect's"""
    if cls == MN:
        return K.HQ_LOSE_MN_ROOT
    if cls == PF:
        return K.HQ_LOSE_PREFILLED
    if redirect:
        return K.HQ_LOSE_REDIRECT
    return K.HQ_LOSE_RUNNING if run else K.HQ_LOSE_ASSIGNED


def test_the_rule_over_its_full_table():
    lib = _debug_lib()
    assert [getattr(abi, k) for k in KINDS] == list(KINDS.values()) == list(range(5))
    assert set(abi.HQ_LOSE_RUNNING_TASKS) == {K.HQ_LOSE_RUNNING, K.HQ_LOSE_MN_ROOT}
    rows = list(itertools.product((SN, MN, PF), (0, 1), (0, 1)))
    assert len(rows) == 12
    cols = [np.ascontiguousarray([r[k] for r in rows], np.uint8) for k in range(3)]
    kind = np.full(len(rows), 255, np.uint8); running = np.full(len(rows), 255, np.uint8)
    p = lambda a: a.ctypes.data_as(abi.u8p)
    assert lib.hqtick_debug_lose_kind(len(rows), *[p(c) for c in cols], p(kind), p(running)) == len(rows)
    assert kind.tolist() == [_restated(*r) for r in rows]
    assert set(kind.tolist()) == set(range(5))  # every kind occurs
    assert running.tolist() == [int(k in abi.HQ_LOSE_RUNNING_TASKS) for k in kind.tolist()]
    # bad arguments
    z = np.zeros(1, np.uint8); bad = np.full(1, 3, np.uint8); out = np.full(1, 255, np.uint8)
    assert lib.hqtick_debug_lose_kind(1, p(bad), p(z), p(z), p(out), None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_lose_kind(1, None, p(z), p(z), p(out), None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_lose_kind(1, p(z), p(z), p(z), None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_lose_kind(1, p(z), p(z), p(z), p(out), None) == 1 and out.tolist() == [K.HQ_LOSE_ASSIGNED]  # (the running column is optional)
    assert lib.hqtick_debug_lose_kind(0, None, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------- the grouping
def _group(lib, ids, prio, rq, kind, widx, n, order):
    k = len(ids)
    off = np.full(n + 1, 0xDEAD, np.uint32); o_id = np.zeros(k, np.uint64); o_pr = np.zeros(k, np.uint64); o_rq = np.zeros(k, np.uint32); o_kind = np.zeros(k, np.uint8)
    ptr = lambda a, t: a.ctypes.data_as(t) if len(a) else None
    got = lib.hqtick_debug_lose_group(k, n, ptr(ids, abi.u64p), ptr(prio, abi.u64p), ptr(rq, abi.u32p), ptr(kind, abi.u8p), ptr(widx, abi.u32p), order,
                                      off.ctypes.data_as(abi.u32p), ptr(o_id, abi.u64p), ptr(o_pr, abi.u64p), ptr(o_rq, abi.u32p), ptr(o_kind, abi.u8p))
    return got, off, o_id, o_pr, o_rq, o_kind


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 255, 256, 257])
def test_the_grouping_against_a_stable_argsort(k, n):
    lib = _debug_lib()
    rng = np.random.default_rng([k, n, 5])
    ids = np.cumsum(rng.integers(1, 9, k)).astype(np.uint64)  # strictly ascending
    prio = rng.integers(0, 2**62, k).astype(np.uint64); rq = rng.integers(0, 2**31, k).astype(np.uint32); kind = rng.integers(0, 5, k).astype(np.uint8)
    widx = rng.integers(0, n, k).astype(np.uint32)
    if n == 5 and k:
        widx[widx == 3] = 2  # (a worker in the middle that holds nothing)
    perm = np.argsort(widx, kind="stable")
    want_off = np.searchsorted(widx[perm], np.arange(n + 1), side="left").astype(np.uint32)
    for order in (0, 1, 2):
        got, off, o_id, o_pr, o_rq, o_kind = _group(lib, ids, prio, rq, kind, widx, n, order)
        assert got == k
        assert off.tolist() == want_off.tolist() and off[0] == 0 and off[n] == k
        assert o_id.tolist() == ids[perm].tolist() and o_pr.tolist() == prio[perm].tolist() and o_rq.tolist() == rq[perm].tolist() and o_kind.tolist() == kind[perm].tolist()
        for w in range(n):  # ids ascend inside a worker
            assert (np.diff(o_id[off[w]:off[w + 1]].astype(np.int64)) > 0).all()


def test_the_grouping_refuses_bad_arguments():
    lib = _debug_lib()
    ids = np.array([3, 5], np.uint64); z64 = np.zeros(2, np.uint64); z32 = np.zeros(2, np.uint32); z8 = np.zeros(2, np.uint8)
    assert _group(lib, ids, z64, z32, z8, np.array([0, 2], np.uint32), 2, 0)[0] == abi.HQTICK_E_INVALID      # an index not below n_workers
    assert _group(lib, ids[::-1].copy(), z64, z32, z8, z32, 2, 0)[0] == abi.HQTICK_E_INVALID                  # ids that do not ascend
    assert _group(lib, ids, z64, z32, z8, z32, 2, 3)[0] == abi.HQTICK_E_INVALID                               # an order outside 0..2
    assert lib.hqtick_debug_lose_group(0, 0, None, None, None, None, None, 0, z32.ctypes.data_as(abi.u32p), None, None, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_lose_group(2, 2, None, None, None, None, None, 0, z32.ctypes.data_as(abi.u32p), None, None, None, None) == abi.HQTICK_E_INVALID


def test_host_functions_under_sanitizers():
    """tools/lose_core_asan.cpp: the rule, the grouping for 0 .. 1030 entries over 1 .. 300 workers and the two buffer layouts, every array in an exact-size heap
    block, under AddressSanitizer + UBSan.  A stand-alone program: nothing is loaded into this process."""
    import tempfile

    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "lose_core_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                               os.path.join(ROOT, "tools", "lose_core_asan.cpp")])
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "lose_core_asan:" in p.stdout and "checks" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- one worker: remove_worker exactly
class _Twin:
    """a device side for the lifecycle driver that, at every loss, plays lose_workers([w]) on a copy of the mirror as it was before and compares; the copy is
    taken ahead of a "lose" step only (_play_with_twin), so the 60-round histories cost a copy per loss, not per step"""

    def __init__(self):
        self.before, self.n = None, 0

    def seed(self, e): pass
    def tick(self, e, snap, want, code): return want
    def refused(self, e, which): pass
    def consume(self, e, want): pass
    def new_tasks(self, e, ids, deps): pass
    def disposed(self, e, msgs): pass
    def start(self, e, triples, accepted): pass
    def finish(self, e, pairs, released): pass
    def fail(self, e, pairs, accepted): pass
    def cancel(self, e, ids, messages, closure): pass
    def retract(self, e, wid, ids, want, n_left): pass
    def add_worker(self, e, wid): pass
    def end(self, e): pass

    def check(self, e): pass

    def lose(self, e, wid, info):
        twin = self.before
        assert twin is not None and wid in twin.workers
        n = twin.lose_workers([wid])
        assert ls.mirror_state(twin) == ls.mirror_state(e)
        assert twin.last_lose_reassigned == info["sent"]
        (rows,) = twin.last_lose_per_worker
        assert [x[0] for x in rows if x[3] in abi.HQ_LOSE_RUNNING_TASKS] == e.last_lost_running
        assert [x[0] for x in rows if x[3] == abi.HQ_LOSE_PREFILLED] == info["prefilled"]
        back = {x for s in e.ready.values() for x in s} - info["ready_before"] - set(info["disposed"])
        assert [x[0] for x in twin.last_lose_requeued] == sorted(back) == [x[0] for x in rows] and n == len(back)
        assert [x[:3] for x in rows] == twin.last_lose_requeued == [(x, e.tasks[x].rq, e.tasks[x].priority) for x in sorted(back)]
        self.before = None
        self.n += 1


def _play_with_twin(h, oracle, twin):
    """lifecycle_cases.play, with the mirror copied ahead of every "lose" step"""
    h.deps_given, h.inserts = {}, 0
    try:
        for rnd, step in h.steps():
            h.log.append((rnd, step))
            if step[0] == "lose":
                twin.before = copy.deepcopy(h.env)
            if not lc._apply(h, oracle, twin, step):
                h.ended_early = rnd
                break
    except Exception as err:
        raise AssertionError(f"{type(err).__name__}: {err}\n{h.describe()}") from err
    return h


@pytest.mark.parametrize("form", lc.FORMS)
def test_one_lost_worker_is_remove_worker_on_every_lifecycle_history(form):
    oracle = Oracle(abi.make_config(reserve=1, fill_max=2, **lc.CFG), canonical=True)
    losses, long_losses = 0, 0
    assert any(seed >= lc.LONG_FROM for seed in lc.SEEDS[form])
    for seed in lc.SEEDS[form]:  # every seed, the long history included
        twin = _Twin()
        _play_with_twin(lc.history(seed, form), oracle, twin)
        losses += twin.n
        long_losses += twin.n if seed >= lc.LONG_FROM else 0
    print(f"{form}: {losses} losses compared, {long_losses} of them in the long history")
    assert losses >= 10 and long_losses >= 1, (losses, long_losses)


# ---------------------------------------------------------------------------------------------- the batched histories on the mirror
def test_histories_reach_every_line_on_the_mirror_alone():
    cov = {}
    for form in ls.FORMS:
        c = collections.Counter()
        for seed in ls.SEEDS[form]:
            oracle = Oracle(abi.make_config(reserve=1, fill_max=2, **lc.CFG), canonical=True)
            h = ls.play(ls.history(seed, form), oracle)
            assert h.rounds_done >= 3, (form, seed, h.rounds_done)
            c.update(h.cov)
        cov[form] = c
    total = collections.Counter()
    for c in cov.values():
        total.update(c)
    for line in ls.LINES:
        assert total[line] > 0, line
    assert any(total[f"batch of {k}"] for k in (3, 4)) and total["batch of 1"] and total["batch of 2"]
    lines = ls.coverage_lines(cov)
    path = os.path.join(ROOT, "profiles", "lose", "coverage.txt")
    text = "kinds and events of the lost-worker histories (tests/lose_cases.py SEEDS) on the mirror, per form\n" + "\n".join(lines) + "\n"
    print(text)
    if not os.path.exists(path):  # (the table is written once and committed; from then on it is compared: delete the file to write it anew)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "w").write(text)
    assert open(path).read() == text


def test_a_batch_is_the_handler_on_the_states_before_it():
    """old and redirect target lost together: no ComputeTasks message goes to a worker that is gone, whatever the order of the list"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

    for order in ((0, 1), (1, 0)):
        e = SchedEnv()
        ws = [e.new_worker(WB(2)) for _ in range(4)]
        t = e.new_task(TB())
        x = e.tasks[t]; x.state, x.worker = core.RETRACTING, ws[0]
        e.redirects[t] = (ws[1], 0); e.workers[ws[1]].assigned_tasks.add(t)
        e.ready[x.rq].discard(t)
        batch = [ws[k] for k in order]
        assert e.lose_workers(batch) == 1
        assert e.last_lose_reassigned == [] and x.state == core.WAITING and t in e.ready[x.rq] and t not in e.redirects
        assert e.last_lose_per_worker[order.index(1)] == [(t, x.rq, x.priority, abi.HQ_LOSE_REDIRECT)] and e.last_lose_per_worker[order.index(0)] == []
        assert sorted(e.workers) == ws[2:]


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
    for n in ("hqtick_debug_lose_kind", "hqtick_debug_lose_group"):
        assert re.search(r"\bint " + n + r"\(", d) and n not in h


def test_libraries_export_the_new_symbols():
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\s(hqtick_\w+)$", out, flags=re.M))
    for n in NEW:
        assert n in syms, n
    assert not {"hqtick_debug_lose_kind", "hqtick_debug_lose_group"} & syms  # the hooks live in the test library only
    out = subprocess.run(["nm", "-D", "--defined-only", build.TEST_LIB], capture_output=True, text=True, check=True).stdout
    for n in NEW + ["hqtick_debug_lose_kind", "hqtick_debug_lose_group"]:
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


def test_python_bindings_exist_and_null_contexts_are_refused():
    for f in ("lose_workers", "lose_last"):
        assert callable(getattr(tick.Tick, f)), f
    assert callable(core.SchedEnv.lose_workers)
    lib = tick.load()
    lib.hqtick_lose_workers.argtypes = [C.c_void_p, C.c_uint32, abi.u32p]
    ws = (C.c_uint32 * 2)(50, 51)
    assert lib.hqtick_lose_workers(None, 0, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_lose_workers(None, 2, ws) == abi.HQTICK_E_INVALID
    for f, n_args in (("hqtick_lose_last_tasks", 6), ("hqtick_lose_last_requeued", 4), ("hqtick_lose_last_reassigned", 4), ("hqtick_lose_last_mn_left", 4)):
        g = getattr(lib, f)
        g.argtypes = [C.c_void_p] * (n_args + 1)
        assert g(None, *([None] * n_args)) == abi.HQTICK_E_INVALID, f
