"""hqtick_fail_tasks (include/hqtick.h) on the device: the reference's task_failed scenarios through graph + ready set + ledger with prefilled
tracking + the resident Retracting table, every kind in one batch, batch order and the last-ALL rule with a refused and a prefilled position between, the
attribution of a closure to the position that removes it at the smallest shapes that can go wrong, twin contexts (the one call against hqtick_assigned_release /
_unprefill + one hqtick_graph_remove per failed task + hqtick_ready_remove) on random histories checked against SchedEnv.fail_tasks, and the call's rules."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cancel_cases as cc
import fail_cases as fl
import test_gpu_finish as gf
from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

pytestmark = pytest.mark.gpu

K = abi
NO = abi.HQ_NO_WORKER
ACC = abi.HQ_FAIL_ACCEPTED
CFG = fl.CFG


def _lists(got):
    off = got["consumer_off"].tolist()
    return [got["consumer_id"][off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def _fail_checked(a, e, pairs, overfull=False, audit=True):
    """the batch on the mirror and on context a, the audit clean before and after: kinds, accepted and refused counts, the consumer lists per position, the graph's
    last ids, ready count, free rows and Retracting count must agree with the mirror"""
    if audit:
        gf._clean(a)
    n_acc = e.fail_tasks(pairs)
    kinds, lists = e.last_fail_kinds, e.last_fail_consumers
    got = a.fail_tasks([p[0] for p in pairs], [p[1] for p in pairs])
    print("kinds", got["kind"].tolist(), "accepted", got["accepted"], "off", got["consumer_off"].tolist()[:40], "removed", len(got["removed"]))
    assert got["kind"].tolist() == kinds
    assert got["accepted"] == n_acc == sum(k in ACC for k in kinds) and a.assigned_last_unknown() == len(pairs) - n_acc
    assert len(got["consumer_off"]) == len(pairs) + 1 and got["consumer_off"][0] == 0
    assert _lists(got) == lists
    roots = [p[0] for p, k in zip(pairs, kinds) if k in ACC]
    assert got["removed"].tolist() == sorted(roots + [c for l in lists for c in l]) and got["graph_unknown"] == 0
    assert a.ready_count() == gf._ready_total(e)
    assert (a.assigned_free_rows() == cc.free_rows(e)).all()
    assert a.retracting_count() == sum(1 for t in e.tasks.values() if t.state == core.RETRACTING)
    if overfull:
        assert set(a.resident_check(gf.AUDIT)["failed"]) == {"HQ_INV_LEDGER_FREE"}
    elif audit:
        gf._clean(a)
    return got


def _tick_ctx(**kw):
    from hyperqueue_amd.tick import Tick

    return Tick(abi.make_config(**dict(CFG, **kw)))


# ---------------------------------------------------------------------------------------------- the reference's scenarios
def test_running_task_on_error():
    a = _tick_ctx()
    try:
        e, ws, wf = fl.scenario_running_task_on_error()
        fl.seed_context(a, e)
        got = _fail_checked(a, e, [(wf[2], ws[2])])
        fl.check_running_task_on_error(e, ws, wf)
        assert got["accepted"] == 1 and a.assigned_count() == 0 and a.assigned_lookup([wf[2]])[0].tolist() == [NO]
        assert a.graph_unfinished([wf[2], wf[3], wf[4], wf[5], wf[6]]).tolist() == [0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
        gf._ready_is(a, e)
    finally:
        a.close()


def test_task_mn_fail():
    a = _tick_ctx()
    try:
        e, t1, root, other = fl.scenario_mn_fail()
        fl.seed_context(a, e)
        assert a.assigned_mn_count() == 1
        got = _fail_checked(a, e, [(t1, other), (t1, NO), (t1, root), (t1, root), (t1, other)])
        assert got["kind"].tolist() == [K.HQ_FAIL_WRONG_WORKER, K.HQ_FAIL_NOT_WAITING, K.HQ_FAIL_MN, K.HQ_FAIL_REPEAT, K.HQ_FAIL_WRONG_WORKER]
        fl.check_mn_fail(e, t1)
        assert a.assigned_mn_count() == 0 and all(f & abi.HQ_WORKER_SN for f in a.cluster_worker_flags().tolist())
        gf._ledger_matches(a, e)
    finally:
        a.close()


def test_prefill_failed():
    a = _tick_ctx(reserve=1, fill_max=1)
    try:
        e = SchedEnv(abi.make_config(reserve=1, fill_max=1, **CFG))
        tasks = e.new_tasks(3, TB())
        w1 = e.new_worker(WB(1))
        snap = e.snapshot()
        a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
        e.apply(gf._tick(a, snap))
        t1 = next(x for x in tasks if e.task(x).is_assigned()); t2 = next(x for x in tasks if e.task(x).is_prefilled())
        cc.seed_ready_graph(a, e)
        assert a.assigned_prefilled_count() == 1
        e.finish_tasks([(t1, w1)])
        assert a.finish_tasks([t1], [w1])["kind"].tolist() == [K.HQ_FINISH_ASSIGNED]
        got = _fail_checked(a, e, [(t2, w1)])  # one call: no hqtick_assigned_unprefill beside it
        fl.check_prefill_failed(e, w1, t1, t2)
        assert got["kind"].tolist() == [K.HQ_FAIL_PREFILLED] and a.assigned_prefilled_count() == 0 and a.assigned_count() == 0
        gf._ledger_matches(a, e)
        gf._next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


def test_steal_failed():
    """test_reactor.rs:1051.  Fails on the parent commit: the symbol does not exist there, and the call sequence the parent documents for task_failed
    (hqtick_assigned_release + hqtick_graph_remove) leaves the failed task's entry in the Retracting table, redirect included -- hqtick_retracting_count stays 1
    where this test wants 0."""
    a = _tick_ctx(reserve=1, fill_max=1)
    try:
        e, w1, w2, t, others = gf._retracting_pair(a)
        cc.seed_ready_graph(a, e)
        (on_w1,) = sorted(e.workers[w1].assigned_tasks)
        before = e.workers[w2].free[0]
        e.finish_tasks([(on_w1, w1)])
        assert a.finish_tasks([on_w1], [w1])["accepted"] == 1
        assert a.assigned_lookup([t])[0].tolist() == [w2] and a.retracting_count() == 1  # the ledger names the redirect TARGET
        got = _fail_checked(a, e, [(t, w2)])  # the target never got the task: refused, nothing changes
        assert got["kind"].tolist() == [K.HQ_FAIL_WRONG_WORKER] and a.retracting_count() == 1 and a.assigned_lookup([t])[0].tolist() == [w2]
        got = _fail_checked(a, e, [(t, w1)])
        fl.check_steal_failed(e, w1, w2, t, before)
        assert got["accepted"] == 1 and a.retracting_count() == 0 and a.assigned_lookup([t])[0].tolist() == [NO]
        assert a.graph_unfinished([t]).tolist() == [0xFFFFFFFF]
        assert a.retract_response(w1, [t]) == []
        gf._next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


def test_worker_crashing_task_at_its_limit():
    a = _tick_ctx()
    try:
        e, w, t1 = fl.scenario_crash_limit()
        fl.seed_context(a, e)
        assert a.ready_count() == 0 and a.assigned_count() == 1
        assert e.remove_worker(w) == [] and a.cluster_remove_workers([w]) == []
        assert a.ready_count() == 1 and a.assigned_count() == 0  # back in its queue
        got = _fail_checked(a, e, [(t1, NO)])
        assert got["kind"].tolist() == [K.HQ_FAIL_WAITING] and a.ready_count() == 0 and a.graph_unfinished([t1]).tolist() == [0xFFFFFFFF]
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- every kind in one batch
def _kinds_batch(e, ws, t):
    w1, w2, w3, root, node = ws
    sn = t["sn"]
    pairs = [(sn[0], root), (sn[0], w3), (t["red"], w2), (t["red"], w1), (10**12, w1), (sn[0], w3), (t["pf"], w3), (t["q"], w3), (t["c_two"], NO), (t["waiting"], NO),
             (t["waiting"], NO), (sn[2], NO), (t["mn"], node), (t["mn"], root), (t["c_ref"], NO), (t["waiting"], w3)]
    want = [K.HQ_FAIL_WRONG_WORKER, K.HQ_FAIL_ASSIGNED, K.HQ_FAIL_WRONG_WORKER, K.HQ_FAIL_RETRACTING, K.HQ_FAIL_NONE, K.HQ_FAIL_REPEAT, K.HQ_FAIL_PREFILLED,
            K.HQ_FAIL_RETRACTING, K.HQ_FAIL_GONE, K.HQ_FAIL_WAITING, K.HQ_FAIL_REPEAT, K.HQ_FAIL_NOT_WAITING, K.HQ_FAIL_WRONG_WORKER, K.HQ_FAIL_MN, K.HQ_FAIL_WAITING,
            K.HQ_FAIL_NONE]
    return pairs, want


def test_every_kind_in_one_batch():
    a = _tick_ctx(reserve=1, fill_max=1)
    try:
        e, ws, t = gf._kinds_env(a, None)
        pairs, want = _kinds_batch(e, ws, t)
        got = _fail_checked(a, e, pairs)
        assert got["kind"].tolist() == want and set(want) == set(range(10))
        lists = _lists(got)
        assert lists[1] == sorted([t["c_acc"], t["c_two"]]) and lists[3] == [t["c_retr"]] and lists[7] == [] and sum(map(len, lists)) == 3
        assert a.retracting_count() == 0 and a.assigned_prefilled_count() == 0 and a.assigned_mn_count() == 0
        assert a.graph_unfinished([t["sn"][2], t["sn"][1]]).tolist() == [0, 0]  # refused or not in the batch: still in the graph
        gf._ledger_matches(a, e)
        gf._ready_is(a, e)
    finally:
        a.close()


def test_audit_mode_runs_the_kinds_batch():
    """a context created with HQTICK_CHECK_RESIDENT=1 audits itself after every call: the kinds batch returns >= 0 (a child process: the variable is read when the
    library creates the context)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_fail as g\nimport test_gpu_finish as gf\nfrom hyperqueue_amd import abi\nfrom hyperqueue_amd.tick import Tick\n"
            "a = Tick(abi.make_config(reserve=1, fill_max=1, **g.CFG))\n"
            "e, ws, t = gf._kinds_env(a, None)\npairs, want = g._kinds_batch(e, ws, t)\n"
            "got = a.fail_tasks([p[0] for p in pairs], [p[1] for p in pairs])\n"
            "assert got['accepted'] == 7 and got['kind'].tolist() == want, got\na.close()\nprint('AUDITED-OK')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HQTICK_CHECK_RESIDENT="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "AUDITED-OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- batch order and the last-ALL rule
@pytest.mark.parametrize("order", ["amount_first", "all_first", "mixed"])
def test_fail_batch_is_applied_in_its_order_with_a_refused_and_a_prefilled_position_between(order):
    e, wid, other, amt, al = gf._one_worker_env()
    pf = e.new_task(TB().cpus(1))
    y = e.tasks[pf]; y.state, y.worker = core.PREFILLED, wid
    e.workers[wid].prefilled_tasks.add(pf); e.ready[y.rq].discard(pf)
    e.prefill[y.rq] = (y.priority, core.task_id_set()); e.prefill[y.rq][1].insert(pf)
    seq = {"amount_first": amt + [al], "all_first": [al] + amt, "mixed": [amt[0], al, amt[1], amt[2]]}[order]
    # the refused (ALL or AMOUNT, other worker) position must not count as the last ALL, and the prefilled one touches no free row
    pairs = [(seq[0], wid), (seq[1], other), (pf, wid), (10**12, wid)] + [(x, wid) for x in seq[1:]]
    t = _tick_ctx()
    try:
        snap = e.snapshot()
        fl.seed_context(t, e)
        assert t.assigned_prefilled_count() == 1
        got = _fail_checked(t, e, pairs, overfull=order != "amount_first")
        assert got["accepted"] == 5 and t.assigned_count() == 0 and t.assigned_prefilled_count() == 0
        total = int(np.asarray(snap.worker_total, np.uint64).reshape(-1)[0])
        expect = {"amount_first": total, "all_first": total + 3 * 10_000, "mixed": total + 2 * 10_000}[order]
        assert int(t.assigned_free_rows()[0, 0]) == expect
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------- attribution shapes
@pytest.mark.parametrize("name", sorted(fl.shapes()))
def test_attribution_shapes(name):
    """kinds, consumer CSR, graph_last_ids, ready count, free rows and Retracting count against the mirror.  Fails on the parent commit (no such symbol); the
    parent's hqtick_graph_remove returns the union of the closures alone."""
    e, pairs = fl.shapes()[name]
    a = _tick_ctx()
    try:
        fl.seed_context(a, e)
        got = _fail_checked(a, e, pairs)
        assert a.graph_stats()["n_tasks"] == sum(1 for t in e.tasks.values() if t.state != core.FINISHED)
        gf._ledger_matches(a, e)
        gf._ready_is(a, e)
    finally:
        a.close()


def test_a_held_root_inside_an_earlier_closure_is_reported():
    """cannot occur on a state hqtick_resident_check accepts: B is assigned although its producer A is still here.  Both fail in one batch: every step completes by
    the smallest-position rule (B is A's consumer, both entries leave the ledger) and the call returns HQTICK_E_INVALID, naming B"""
    from hyperqueue_amd.tick import HqTickError

    e = SchedEnv(abi.make_config(**CFG))
    ws = e.new_workers_cpus([4, 4])
    ta = e.new_task(TB().cpus(1)); tb = e.new_task(TB().cpus(1)); tc = e.new_task(TB().cpus(1).task_deps([tb]))
    e.assign_task(ta, ws[0]); e.assign_task(tb, ws[1])
    a = _tick_ctx()
    try:
        fl.seed_context(a, e)
        x = e.tasks[tb]
        a.graph_remove([tb, tc], True)
        assert a.graph_add_tasks([tb, tc], [x.priority, x.priority], [x.rq, x.rq], [[ta], [tb]]).tolist() == []  # now B waits for A in the graph
        with pytest.raises(HqTickError) as err:
            a.fail_tasks([ta, tb], [ws[0], ws[1]])
        assert err.value.code == abi.HQTICK_E_INVALID and str(tb) in str(err.value)
        got = a.fail_last()
        assert got["kind"].tolist() == [K.HQ_FAIL_ASSIGNED, K.HQ_FAIL_ASSIGNED] and _lists(got) == [[tb, tc], []] and got["removed"].tolist() == [ta, tb, tc]
        assert a.assigned_count() == 0 and a.graph_stats()["n_tasks"] == 0
        total = np.asarray(e.snapshot().worker_total, np.uint64).reshape(2, -1)
        assert (a.assigned_free_rows() == total).all()
    finally:
        a.close()


def test_without_a_graph_waiting_ids_just_leave_the_ready_set():
    e = SchedEnv(abi.make_config(**CFG))
    ws = e.new_workers_cpus([4, 4])
    held, r1, r2 = e.new_task(TB().cpus(1)), e.new_task(TB().cpus(1)), e.new_task(TB().cpus(1))
    e.assign_task(held, ws[0])
    a = _tick_ctx()
    try:
        fl.seed_context(a, e, graph=False)
        pairs = [(r1, NO), (r1, NO), (held, ws[0]), (r2, ws[0]), (held, NO)]
        e.fail_tasks(pairs)
        got = a.fail_tasks([p[0] for p in pairs], [p[1] for p in pairs])
        assert got["kind"].tolist() == e.last_fail_kinds == [K.HQ_FAIL_WAITING, K.HQ_FAIL_REPEAT, K.HQ_FAIL_ASSIGNED, K.HQ_FAIL_NONE, K.HQ_FAIL_NOT_WAITING]
        assert got["accepted"] == 2 and a.assigned_last_unknown() == 3 and got["consumer_off"].tolist() == [0] * 6 and len(got["removed"]) == 0
        assert a.ready_count() == 1 and a.assigned_count() == 0 and (a.assigned_free_rows() == cc.free_rows(e)).all()
        assert a.ready_remove([r2]) == 1
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- twin contexts on random histories
@pytest.mark.parametrize("seed", list(fl.HISTORY_SEEDS))
def test_twin_contexts_on_a_random_history(seed):
    """context A fails the batch with the one call; context B takes the parent's sequence per accepted position, in order: hqtick_assigned_release or
    hqtick_assigned_unprefill, hqtick_graph_remove([id], 1), hqtick_ready_remove.  Each single removal minus its root is A's list of that position; afterwards
    both show the same ledger, graph and ready set.  B has no call that drops a failed task's Retracting entry: its table keeps them (what the one call is for),
    so the table is compared with the mirror on A alone."""
    from hyperqueue_amd.tick import Tick

    e, pairs = fl.history(seed)
    a, b = Tick(e.config), Tick(e.config)
    try:
        for t in (a, b):
            fl.seed_context(t, e)
        ever = sorted(e.tasks)
        got = _fail_checked(a, e, pairs)
        lists = _lists(got)
        n_retr = 0
        for i, ((tid, wid), kind) in enumerate(zip(pairs, got["kind"].tolist())):
            if kind not in ACC:
                continue
            if kind in (K.HQ_FAIL_ASSIGNED, K.HQ_FAIL_MN):
                assert b.assigned_release([tid]) == 1
            elif kind == K.HQ_FAIL_PREFILLED:
                assert b.assigned_unprefill([tid]) == 1
            n_retr += kind == K.HQ_FAIL_RETRACTING
            rem = b.graph_remove([tid], True).tolist()
            assert tid in rem and [x for x in rem if x != tid] == lists[i]
            b.ready_remove(rem)
        assert b.retracting_count() == a.retracting_count() + n_retr
        va, vb = (dict(ready=t.ready_count(), sn=t.assigned_count(), pf=t.assigned_prefilled_count(), mn=t.assigned_mn_count(), free=t.assigned_free_rows().tolist(),
                       worker=t.assigned_lookup(ever)[0].tolist(), unf=t.graph_unfinished(ever).tolist(), tasks=t.graph_stats()["n_tasks"]) for t in (a, b))
        assert va == vb
        assert va["unf"] == [0xFFFFFFFF if e.tasks[x].state == core.FINISHED else e.tasks[x].unfinished_deps for x in ever]
        gf._ledger_matches(a, e)
        gf._ready_is(a, e)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- the call's rules
def test_call_rules():
    from hyperqueue_amd.tick import HqTickError, Tick

    a = Tick(abi.make_config(**CFG))
    try:
        e = SchedEnv(abi.make_config(**CFG))
        ws = e.new_workers_cpus([4, 4])
        held = [e.new_task(TB().cpus(1)) for _ in range(2)]
        e.assign_task(held[0], ws[0]); e.assign_task(held[1], ws[1])
        queued = [e.new_task(TB().cpus(1)) for _ in range(5)]
        cons = e.new_task(TB().cpus(1).task_deps([held[0]]))
        with pytest.raises(HqTickError) as err:  # no resident ready set
            a.fail_tasks(held, ws)
        assert err.value.code == abi.HQTICK_E_INVALID
        a.cluster_upload(e.snapshot())
        cc.seed_ready_graph(a, e)
        before = gf._state(a)
        with pytest.raises(HqTickError) as err:  # ledger off
            a.fail_tasks(held, ws)
        assert err.value.code == abi.HQTICK_E_INVALID and "assignment ledger not enabled" in str(err.value)
        assert gf._state(a) == before
        cc.seed_ledger(a, e)
        free = a.assigned_free_rows().copy()
        got = a.fail_tasks([], [])  # n = 0: empty lists
        assert got["accepted"] == 0 and len(got["kind"]) == 0 and got["consumer_off"].tolist() == [0] and a.assigned_last_unknown() == 0
        f = a._lib.hqtick_fail_tasks
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p]
        ids = np.asarray(held, np.uint64); wid = np.asarray(ws, np.uint32)
        assert f(a._ctx, 2, ids.ctypes.data_as(abi.u64p), None) == abi.HQTICK_E_INVALID  # a null array
        assert f(a._ctx, 2, None, wid.ctypes.data_as(abi.u32p)) == abi.HQTICK_E_INVALID
        assert f(a._ctx, (1 << 26) + 1, ids.ctypes.data_as(abi.u64p), wid.ctypes.data_as(abi.u32p)) == abi.HQTICK_E_CAPACITY  # (refused before an array is read)
        assert f(a._ctx, 0, None, None) == 0
        assert gf._state(a) == before and (a.assigned_free_rows() == free).all() and a.assigned_count() == 2
        # a two-call tick's placement is pending: refused, nothing changes, and the consume still finds its selection
        res = gf._tick(a, e.snapshot(), resident=True)
        assert sum(len(r) for r in res.records) == 5
        pending = gf._state(a)
        with pytest.raises(HqTickError) as err:
            a.fail_tasks(held, ws)
        assert err.value.code == abi.HQTICK_E_INVALID and "pending" in str(err.value)
        assert gf._state(a) == pending and (a.assigned_free_rows() == free).all() and a.assigned_count() == 2 and a.assigned_lookup(held)[0].tolist() == ws
        a.ready_consume_last()
        e.apply(res)
        assert a.ready_count() == 0 and a.assigned_count() == 7
        got = _fail_checked(a, e, [(held[0], ws[0]), (held[1], ws[0]), (queued[0], e.tasks[queued[0]].worker)])
        assert got["accepted"] == 2 and _lists(got) == [[cons], [], []] and a.assigned_count() == 5
        # the arrays stay valid until the next hqtick_fail_tasks: other calls in between do not move or change them
        n = C.c_uint32(); pk = abi.u8p(); po = abi.u32p(); pi = abi.u64p()
        a._lib.hqtick_fail_last_routes(a._ctx, C.byref(n), C.byref(pk)); a._lib.hqtick_fail_last_consumers(a._ctx, C.byref(n), C.byref(po), C.byref(pi))
        e.finish_tasks([(held[1], ws[1])])
        assert a.finish_tasks([held[1]], [ws[1]])["accepted"] == 1
        a.graph_remove([queued[1]], True); a.assigned_release([queued[1]]); gf._clean(a)
        again = a.fail_last()
        assert again["kind"].tolist() == got["kind"].tolist() and _lists(again) == [[cons], [], []]
        assert abi._np(pk, 3, np.uint8).tolist() == got["kind"].tolist() and abi._np(po, 4, np.uint32).tolist() == [0, 1, 1, 1] and abi._np(pi, 1, np.uint64).tolist() == [cons]
    finally:
        a.close()


def test_the_same_batch_on_a_fresh_identical_context_gives_byte_equal_outputs():
    from hyperqueue_amd.tick import Tick

    outs = []
    for _ in range(2):
        e, pairs = fl.history(3)
        a = Tick(e.config)
        try:
            fl.seed_context(a, e)
            got = a.fail_tasks([p[0] for p in pairs], [p[1] for p in pairs])
            outs.append((got["accepted"], got["kind"].tobytes(), got["consumer_off"].tobytes(), got["consumer_id"].tobytes(), got["removed"].tobytes()))
        finally:
            a.close()
    assert outs[0] == outs[1] and len(outs[0][3]) > 0
    e, pairs = fl.shapes()["fan_of_300"]
    for _ in range(2):
        e, pairs = fl.shapes()["fan_of_300"]
        a = Tick(e.config)
        try:
            fl.seed_context(a, e)
            got = a.fail_tasks([p[0] for p in pairs], [p[1] for p in pairs])
            outs.append((got["kind"].tobytes(), got["consumer_off"].tobytes(), got["consumer_id"].tobytes()))
        finally:
            a.close()
    assert outs[2] == outs[3]
