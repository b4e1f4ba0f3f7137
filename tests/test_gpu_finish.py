"""hqtick_finish_tasks and hqtick_retracting_started (include/hqtick.h) on the device: the reference's finish scenarios through graph + ready set +
ledger with prefilled tracking + the resident Retracting table, every kind in one batch, the last-ALL rule with a refused position, the graph's skip input at
wave and workgroup edges, consumer runs of every release path, twin contexts (the one call against today's hqtick_assigned_release + hqtick_graph_finish of the
accepted ids) on random histories checked against SchedEnv.finish_tasks, the call's rules, the audit mode and one larger batch."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import cancel_cases as cc
import finish_cases as fc
import resident_checks as rc
from hyperqueue_amd import abi, core, workloads
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

pytestmark = pytest.mark.gpu

AUDIT = abi.HQ_CHECK_ALL | abi.HQ_CHECK_STRICT
CFG = dict(time_limit_s=20.0)
ACC = abi.HQ_FINISH_ACCEPTED
F = abi


def _strip(snap):
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None; sc.prefilled_off = None; sc.prefilled_rq = None
    sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None
    sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
    return sc


def _tick(t, snap, resident=False):
    """a tick of a ledger context: resident workers and Retracting table, no assigned and no prefilled CSR; resident: on the resident ready set (two-call form)"""
    return abi.parse_result(t.tick_raw(_strip(snap), resident=resident), len(snap.worker_id), snap.n_resources)


def _clean(t):
    r = t.resident_check(AUDIT)
    assert r["n_failed"] == 0, r["failed"]
    return r


def _ready_total(e):
    return sum(len(s) for s in e.ready.values())


def _finish_checked(a, e, pairs, overfull=False):
    """the batch on the mirror and on context a, the audit clean before and after: kinds, accepted count, refused count, released consumers, ready count and
    free rows must agree.  overfull: the batch releases an ALL entry before AMOUNT entries of the same worker, which leaves free > total in the reference too
    (workerload.rs:194-202) -- the audit's HQ_INV_LEDGER_FREE says so, and must be the only invariant that speaks"""
    _clean(a)
    want = e.finish_tasks(pairs)
    kinds = e.last_finish_kinds
    got = a.finish_tasks([p[0] for p in pairs], [p[1] for p in pairs])
    print("kinds", got["kind"].tolist(), "accepted", got["accepted"], "released", got["released"].tolist())
    assert got["kind"].tolist() == kinds
    n_acc = sum(k in ACC for k in kinds)
    assert got["accepted"] == n_acc and a.assigned_last_unknown() == len(pairs) - n_acc
    assert got["released"].tolist() == sorted(want) and got["graph_unknown"] == 0
    assert a.ready_count() == _ready_total(e)
    assert (a.assigned_free_rows() == cc.free_rows(e)).all()
    if overfull:
        assert set(a.resident_check(AUDIT)["failed"]) == {"HQ_INV_LEDGER_FREE"}
    else:
        _clean(a)
    return got


_ledger_matches = rc.ledger_matches  # (tests/resident_checks.py)


def _ready_is(a, e):
    """the resident ready set holds exactly the mirror's ids (destructive: the ids are removed one batch, and nothing may be left)"""
    ready = sorted(x for s in e.ready.values() for x in s)
    assert a.ready_count() == len(ready)
    if ready:
        assert a.ready_remove(ready) == len(ready)
    assert a.ready_count() == 0


# ---------------------------------------------------------------------------------------------- the reference's scenarios
def test_assignments_and_finish():
    from hyperqueue_amd.tick import Tick

    a = Tick(abi.make_config(**CFG))
    try:
        e, ws, steps, t = fc.scenario_assignments_and_finish()
        cc.seed_ledger(a, e); a.assigned_track_prefilled([]); cc.seed_ready_graph(a, e)
        for pairs, held, released in steps:
            got = _finish_checked(a, e, pairs)
            assert got["accepted"] == 1 and got["released"].tolist() == released
            lw, _ = a.assigned_lookup(sorted(e.tasks))
            assert {w: {x for x, y in zip(sorted(e.tasks), lw.tolist()) if y == w} for w in ws} == held
        assert a.assigned_count() == 0 and a.retracting_count() == 0
        assert a.graph_unfinished([t["t3"], t["t7"]]).tolist() == [0, 1]
        snap = e.snapshot()
        res = _tick(a, snap, resident=True)
        a.ready_consume_last(); e.apply(res)  # (apply checks the tick's free rows against the mirror's)
        assert e.tasks[t["t3"]].is_assigned()  # test_reactor.rs:279-286
        _ledger_matches(a, e); _clean(a)
    finally:
        a.close()


def test_mn_finish_by_its_root():
    from hyperqueue_amd.tick import Tick

    a = Tick(abi.make_config(**CFG))
    try:
        e, t1, root, other = fc.scenario_mn_finish()
        cc.seed_ledger(a, e); a.assigned_track_prefilled([]); cc.seed_ready_graph(a, e)
        assert a.assigned_mn_count() == 1
        got = _finish_checked(a, e, [(t1, other), (t1, root), (t1, root), (t1, other)])
        assert got["kind"].tolist() == [F.HQ_FINISH_WRONG_WORKER, F.HQ_FINISH_MN, F.HQ_FINISH_REPEAT, F.HQ_FINISH_WRONG_WORKER]
        assert a.assigned_mn_count() == 0 and all(f & abi.HQ_WORKER_SN for f in a.cluster_worker_flags().tolist())
        _ledger_matches(a, e)
        assert (_tick(a, e.snapshot()).new_free == cc.free_rows(e)).all()
    finally:
        a.close()


def _retracting_pair(a):
    """test_reactor.rs:993-1007 with context a as the scheduler AND the ledger host (as tests/test_gpu_cancel.py builds it):
    -> (mirror, w1, w2, the Retracting task, the other two)"""
    e = SchedEnv(abi.make_config(reserve=1, fill_max=1, **CFG))
    tasks = e.new_tasks(3, TB())
    w1 = e.new_worker(WB(1))
    snap = e.snapshot()
    a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
    e.apply(_tick(a, snap))
    w2 = e.new_worker(WB(2))
    s2 = e.snapshot()
    tot = np.asarray(s2.worker_total, np.uint64).reshape(len(s2.worker_id), s2.n_resources)[s2.worker_id.tolist().index(w2)][None, :]
    a.cluster_add_workers([w2], tot, tot)
    e.apply(_tick(a, e.snapshot()))
    (t,) = [x for x in tasks if e.task(x).is_retracting()]
    assert e.task(t).worker == w1 and e.redirects[t][0] == w2 and a.retracting_count() == 1
    return e, w1, w2, t, [x for x in tasks if x != t]


def _next_tick_equals_the_mirrors(a, e):
    """a fresh task arrives (a tick needs a ready task), then one tick on the resident ready set, applied to the mirror"""
    x = e.tasks[e.new_task(TB())]
    assert a.graph_add_tasks([x.id], [x.priority], [x.rq], [[]]).tolist() == [x.id]
    snap = e.snapshot()
    res = _tick(a, snap, resident=True)
    a.ready_consume_last(); e.apply(res)
    _ledger_matches(a, e)
    assert (a.assigned_free_rows() == cc.free_rows(e)).all()
    _clean(a)


def test_steal_finished():
    from hyperqueue_amd.tick import Tick

    a = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))
    try:
        e, w1, w2, t, others = _retracting_pair(a)
        cc.seed_ready_graph(a, e)
        assert a.assigned_lookup([t])[0].tolist() == [w2]  # the ledger names the redirect TARGET
        before = e.workers[w2].free[0]
        got = _finish_checked(a, e, [(t, w2)])  # the target never got the task: refused, nothing changes
        assert got["kind"].tolist() == [F.HQ_FINISH_WRONG_WORKER] and a.retracting_count() == 1 and a.assigned_lookup([t])[0].tolist() == [w2]
        got = _finish_checked(a, e, [(t, w1)])
        fc.check_steal_finished(e, w1, w2, t, before)
        assert got["accepted"] == 1 and a.retracting_count() == 0 and a.assigned_lookup([t])[0].tolist() == [abi.HQ_NO_WORKER]
        assert a.graph_unfinished([t]).tolist() == [0xFFFFFFFF]
        assert a.retract_response(w1, [t]) == []
        _next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


def test_steal_running():
    from hyperqueue_amd.tick import Tick

    a = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))
    try:
        e, w1, w2, t, others = _retracting_pair(a)
        cc.seed_ready_graph(a, e)
        (on_w1,) = sorted(e.workers[w1].assigned_tasks)
        _finish_checked(a, e, [(on_w1, w1)])
        x = e.tasks[t]
        assert a.retracting_started([(t, w2, x.rq, 0, x.priority)]) == 0 and a.assigned_last_unknown() == 1 and a.retracting_count() == 1
        assert e.start_retracting_task(t, w1, 0)
        _clean(a)
        assert a.retracting_started([(t, w1, x.rq, 0, x.priority), (10**9, w1, x.rq, 0, 0)]) == 1 and a.assigned_last_unknown() == 1
        fc.check_steal_running(e, w1, w2, t, on_w1)
        assert a.retracting_count() == 0 and a.assigned_lookup([t])[0].tolist() == [w1]
        assert (a.assigned_free_rows() == cc.free_rows(e)).all()
        _clean(a)
        _next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


@pytest.mark.parametrize("how", ["started", "finished"])
def test_retaken_by_its_own_worker(how):
    """the dummy redirect (reactor.rs:315-322): a prefill set dissolved by a higher-priority arrival leaves its task Retracting{w1} in its queue; the task w1 ran
    finishes and the next tick puts the Retracting task back on w1 itself (HQ_REDIRECT_SAME_WORKER: an entry on w1, no redirect).  Started there: remove first,
    insert second must work.  Finished there: the entry is given back."""
    from hyperqueue_amd.tick import Tick

    a = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))
    try:
        e = SchedEnv(abi.make_config(reserve=1, fill_max=1, **CFG))
        tasks = e.new_tasks(3, TB())
        w1 = e.new_worker(WB(1))
        snap = e.snapshot()
        a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
        e.apply(_tick(a, snap))
        assigned = next(x for x in tasks if e.task(x).is_assigned()); t = next(x for x in tasks if e.task(x).is_prefilled())
        e.new_task(TB().cpus(2).user_priority(10))  # fits no worker; dissolves the prefill set (process_retracted: the host's part)
        assert e.retract_messages == [(w1, t)] and e.task(t).is_retracting()
        assert a.assigned_unprefill([t]) == 1
        a.retracting_add([t], [w1])
        cc.seed_ready_graph(a, e)
        _finish_checked(a, e, [(assigned, w1)])
        res = _tick(a, e.snapshot(), resident=True)
        a.ready_consume_last(); e.apply(res)
        assert res.redirect_kinds == [abi.HQ_REDIRECT_SAME_WORKER] and t in e.retaken_variant and t not in e.redirects
        assert a.assigned_lookup([t])[0].tolist() == [w1] and a.retracting_count() == 1
        x = e.tasks[t]
        if how == "started":
            _clean(a)
            assert e.start_retracting_task(t, w1, 0)
            assert a.retracting_started([(t, w1, x.rq, 0, x.priority)]) == 1 and a.assigned_last_unknown() == 0
            assert a.assigned_lookup([t])[0].tolist() == [w1] and a.assigned_count() == 1
        else:
            got = _finish_checked(a, e, [(t, w1)])
            assert got["kind"].tolist() == [F.HQ_FINISH_RETRACTING] and a.assigned_count() == 0
        assert a.retracting_count() == 0 and (a.assigned_free_rows() == cc.free_rows(e)).all()
        _clean(a)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- every kind in one batch
def _kinds_env(a, b):
    """five workers; on context a: single-node tasks, a two-node task, a prefilled task, a Retracting task with a redirect (w1 -> w2), one without that sits in
    its queue, consumers behind accepted and refused producers.  b: the mirror's scheduler for the setup."""
    e, w1, w2, t_red, others = _retracting_pair(a)
    ws = [w1, w2] + [e.new_worker(WB(4)) for _ in range(3)]
    s = e.snapshot()
    tot = np.asarray(s.worker_total, np.uint64).reshape(len(s.worker_id), s.n_resources)
    a.cluster_add_workers(ws[2:], tot[2:], tot[2:])
    # a two-node task: the only ready task of the next tick, which places it on two of the three free workers (the ledger learns its request with that tick)
    mn = e.new_task(TB().n_nodes(2))
    e.apply(_tick(a, e.snapshot()))
    assert e.tasks[mn].state == core.RUNNING_MN and a.assigned_mn_count() == 1
    root, node = e.tasks[mn].mn_workers
    (w3,) = [w for w in ws[2:] if w not in (root, node)]
    ws = [w1, w2, w3, root, node]
    # plain tasks on w3, entered by hand on both sides
    sn = [e.new_task(TB().cpus(1)) for _ in range(3)]
    for x in sn:
        e.assign_task(x, ws[2])
    a.assigned_add([(x, ws[2], e.tasks[x].rq, 0, e.tasks[x].priority) for x in sn])
    # a Retracting task in its queue, no redirect (as process_retracted leaves it), and a prefilled one
    t_q = e.new_task(TB().cpus(1)); t_pf = e.new_task(TB().cpus(1))
    x = e.tasks[t_q]; x.state, x.worker = core.RETRACTING, ws[2]
    a.retracting_add([t_q], [ws[2]])
    y = e.tasks[t_pf]; y.state, y.worker = core.PREFILLED, ws[2]
    e.workers[ws[2]].prefilled_tasks.add(t_pf); e.ready[y.rq].discard(t_pf)
    e.prefill[y.rq] = (y.priority, core.task_id_set()); e.prefill[y.rq][1].insert(t_pf)
    assert a.assigned_track_prefilled([(t_pf, ws[2], y.rq, y.priority)]) == 1
    # consumers: of an accepted producer, of a refused one, of two producers of the batch
    c_acc = e.new_task(TB().cpus(1).task_deps([sn[0]])); c_ref = e.new_task(TB().cpus(1).task_deps([sn[2]])); c_two = e.new_task(TB().cpus(1).task_deps([sn[0], sn[1]]))
    c_retr = e.new_task(TB().cpus(1).task_deps([t_red, t_q]))
    waiting = e.new_task(TB().cpus(1))
    cc.seed_ready_graph(a, e)
    return e, ws, dict(mn=mn, red=t_red, q=t_q, pf=t_pf, sn=sn, c_acc=c_acc, c_ref=c_ref, c_two=c_two, c_retr=c_retr, waiting=waiting)


def _kinds_batch(e, ws, t):
    w1, w2, w3, w4, w5 = ws
    sn = t["sn"]
    pairs = [(sn[0], w4), (sn[0], w3), (t["red"], w2), (t["red"], w1), (10**12, w1), (sn[0], w3), (t["pf"], w3), (t["q"], w3), (sn[1], w3), (sn[2], w1),
             (t["red"], w1), (t["waiting"], w3), (t["q"], w4), (t["mn"], w5), (t["mn"], w4)]
    want = [F.HQ_FINISH_WRONG_WORKER, F.HQ_FINISH_ASSIGNED, F.HQ_FINISH_WRONG_WORKER, F.HQ_FINISH_RETRACTING, F.HQ_FINISH_NONE, F.HQ_FINISH_REPEAT, F.HQ_FINISH_PREFILLED,
            F.HQ_FINISH_RETRACTING, F.HQ_FINISH_ASSIGNED, F.HQ_FINISH_WRONG_WORKER, F.HQ_FINISH_REPEAT, F.HQ_FINISH_NONE, F.HQ_FINISH_WRONG_WORKER, F.HQ_FINISH_WRONG_WORKER, F.HQ_FINISH_MN]
    return pairs, want


def test_every_kind_in_one_batch():
    from hyperqueue_amd.tick import Tick

    a = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))
    try:
        e, ws, t = _kinds_env(a, None)
        pairs, want = _kinds_batch(e, ws, t)
        n_ready = a.ready_count()
        got = _finish_checked(a, e, pairs)
        assert got["kind"].tolist() == want and set(want) == set(range(7))
        assert got["released"].tolist() == sorted([t["c_acc"], t["c_two"], t["c_retr"]])
        assert a.retracting_count() == 0
        assert a.ready_count() == n_ready - 1 + 3  # the in-queue Retracting id left, three consumers joined
        cons = [t["c_acc"], t["c_ref"], t["c_two"], t["c_retr"]]
        assert a.graph_unfinished(cons).tolist() == [e.tasks[c].unfinished_deps for c in cons] == [0, 1, 0, 0]  # the refused producer's consumer is not decremented
        assert a.graph_unfinished([t["sn"][2], t["pf"], t["waiting"]]).tolist() == [0, 0, 0]  # refused positions: still in the graph
        assert a.graph_unfinished([t["sn"][0], t["red"], t["q"]]).tolist() == [0xFFFFFFFF] * 3
        _ledger_matches(a, e)
        _ready_is(a, e)
    finally:
        a.close()


def test_audit_mode_runs_the_kinds_batch():
    """a context created with HQTICK_CHECK_RESIDENT=1 audits itself after every call: the kinds batch returns >= 0 (a child process: the variable is read when the
    library creates the context)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_finish as g\nfrom hyperqueue_amd import abi\nfrom hyperqueue_amd.tick import Tick\n"
            "a = Tick(abi.make_config(reserve=1, fill_max=1, **g.CFG))\n"
            "e, ws, t = g._kinds_env(a, None)\npairs, want = g._kinds_batch(e, ws, t)\n"
            "got = a.finish_tasks([p[0] for p in pairs], [p[1] for p in pairs])\n"
            "assert got['accepted'] == 5 and got['kind'].tolist() == want, got\na.close()\nprint('AUDITED-OK')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HQTICK_CHECK_RESIDENT="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "AUDITED-OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- the last-ALL rule
def _one_worker_env():
    e = SchedEnv(abi.make_config(**CFG))
    wid, other = e.new_workers_cpus([8, 8])
    amt = [e.new_task(TB().cpus(1)) for _ in range(3)]
    al = e.new_task(TB().cpus_all())
    for x in amt:
        e.assign_task(x, wid)
    e.assign_task(al, wid)  # (by hand: ALL after AMOUNTs, the over-full row the ledger reproduces)
    return e, wid, other, amt, al


@pytest.mark.parametrize("order", ["amount_first", "all_first", "mixed"])
def test_finish_batch_is_applied_in_its_order_with_a_refused_position_between(order):
    from hyperqueue_amd.tick import Tick

    e, wid, other, amt, al = _one_worker_env()
    seq = {"amount_first": amt + [al], "all_first": [al] + amt, "mixed": [amt[0], al, amt[1], amt[2]]}[order]
    pairs = [(seq[0], wid), (seq[1], other), (10**12, wid)] + [(x, wid) for x in seq[1:]]  # the refused (al or amount, other worker) position must not count as the last ALL
    t = Tick(abi.make_config(**CFG))
    try:
        snap = e.snapshot()
        cc.seed_ledger(t, e); t.assigned_track_prefilled([]); cc.seed_ready_graph(t, e)
        got = _finish_checked(t, e, pairs, overfull=order != "amount_first")
        assert got["accepted"] == 4 and t.assigned_count() == 0
        total = int(np.asarray(snap.worker_total, np.uint64).reshape(-1)[0])
        expect = {"amount_first": total, "all_first": total + 3 * 10_000, "mixed": total + 2 * 10_000}[order]
        assert int(t.assigned_free_rows()[0, 0]) == expect
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------- the skip input at wave and workgroup edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_skip_input_at_wave_and_workgroup_edges(n):
    """n positions on two workers; the positions 0, 63, 64, 255, 256 (where they exist) are refused (wrong worker) and their ids appear nowhere else; the twin takes
    hqtick_assigned_release + hqtick_graph_finish of the accepted ids"""
    from hyperqueue_amd.tick import Tick

    e = SchedEnv(abi.make_config(**CFG))
    ws = e.new_workers_cpus([400, 400])
    tasks = [e.new_task(TB().cpus(1)) for _ in range(n)]
    for k, x in enumerate(tasks):
        e.assign_task(x, ws[k % 2])
    cons = [e.new_task(TB().cpus(1).task_deps([x])) for x in tasks]
    refused = [p for p in (0, 63, 64, 255, 256) if p < n]
    pairs = [(x, ws[(k + (k in refused)) % 2]) for k, x in enumerate(tasks)]
    a, b = Tick(e.config), Tick(e.config)
    try:
        for t in (a, b):
            cc.seed_ledger(t, e); t.assigned_track_prefilled([]); cc.seed_ready_graph(t, e)
        got = _finish_checked(a, e, pairs)
        assert [k for k, kind in enumerate(got["kind"].tolist()) if kind not in ACC] == refused
        assert all(got["kind"][k] == F.HQ_FINISH_WRONG_WORKER for k in refused)
        acc_ids = [x for k, x in enumerate(tasks) if k not in refused]
        assert b.assigned_release(acc_ids) == len(acc_ids)
        rel, unknown = b.graph_finish(acc_ids)
        assert unknown == 0 and rel.tolist() == got["released"].tolist() == sorted(c for k, c in enumerate(cons) if k not in refused)
        assert (a.assigned_free_rows() == b.assigned_free_rows()).all() and a.ready_count() == b.ready_count() and a.assigned_count() == b.assigned_count() == len(refused)
        sa, sb = a.graph_stats(), b.graph_stats(); sa.pop("last_kernel_us", None); sb.pop("last_kernel_us", None)
        assert sa == sb
        assert a.graph_unfinished(cons).tolist() == b.graph_unfinished(cons).tolist() == [int(k in refused) for k in range(n)]
        _ready_is(a, e)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- consumer runs
def test_consumer_runs_of_every_release_path():
    """three producers with 4 consumers (a short run), 5 (SHORT_RUN + 1: the deferred list) and 4097 (RUN_CHUNK + 1: two chunks), each with a refused twin position
    in the batch; one consumer fed by two producers of the batch is released exactly once"""
    from hyperqueue_amd.tick import Tick

    e = SchedEnv(abi.make_config(**CFG))
    ws = e.new_workers_cpus([8, 8])
    p4, p5, pbig, pa, pb = [e.new_task(TB().cpus(1)) for _ in range(5)]
    for x in (p4, p5, pbig, pa, pb):
        e.assign_task(x, ws[0])
    cons = {p: [e.new_task(TB().cpus(1).task_deps([p])) for _ in range(k)] for p, k in ((p4, 4), (p5, 5), (pbig, 4097))}
    shared = e.new_task(TB().cpus(1).task_deps([pa, pb]))
    a = Tick(e.config)
    try:
        cc.seed_ledger(a, e); a.assigned_track_prefilled([]); cc.seed_ready_graph(a, e)
        pairs = [(p4, ws[1]), (pbig, ws[0]), (p5, ws[1]), (pa, ws[0]), (p4, ws[0]), (pbig, ws[1]), (p5, ws[0]), (pb, ws[0]), (pa, ws[1])]
        got = _finish_checked(a, e, pairs)
        assert got["accepted"] == 5 and len(got["released"]) == 4 + 5 + 4097 + 1
        assert got["released"].tolist().count(shared) == 1 and a.ready_count() == 4107
        assert not a.graph_unfinished(got["released"]).any()
        _ready_is(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- twin contexts on random histories
def _history_env(rng):
    e = SchedEnv(abi.make_config(reserve=1, fill_max=2, **CFG))
    gpu = e.new_named_resource("gpus")
    for _ in range(int(rng.integers(3, 6))):
        e.new_worker(WB(int(rng.integers(2, 6))).res_sum("gpus", 2))
    shapes = [TB().cpus(1), TB().cpus(2), TB().cpus(3).next_variant().cpus(1), TB().cpus(1).add_resource(gpu, 1), TB().cpus(2).next_variant().cpus(1).add_resource(gpu, 1)]
    roots = [e.new_task(shapes[int(rng.integers(0, len(shapes)))]) for _ in range(40)]
    for _ in range(25):
        deps = [roots[int(k)] for k in rng.choice(len(roots), int(rng.integers(1, 3)), replace=False)]
        roots.append(e.new_task(shapes[int(rng.integers(0, len(shapes)))].task_deps(deps)))
    return e


@pytest.mark.parametrize("seed", range(20))
def test_twin_contexts_on_a_random_history(seed):
    """context A finishes with the one call, context B with today's hqtick_assigned_release + hqtick_graph_finish of the ids the mirror accepts (and
    hqtick_retract_response / hqtick_retracting_* kept in step by hand where the one call touches the table); after every batch both show the same ledger, ready
    count, graph and next tick, and A's kinds are the mirror's"""
    from hyperqueue_amd.tick import HqTickError, Tick

    rng = np.random.default_rng(4100 + seed)
    e = _history_env(rng)
    a, b = Tick(e.config), Tick(e.config)
    try:
        snap = e.snapshot()
        for t in (a, b):
            t.cluster_upload(snap); t.assigned_enable([]); t.assigned_track_prefilled([]); cc.seed_ready_graph(t, e)
        wids = sorted(e.workers)
        batches = 0
        for rnd in range(4):
            snap = e.snapshot()
            try:
                ra = _tick(a, snap, resident=True)
            except HqTickError as err:
                assert err.code == abi.HQTICK_E_UNSUPPORTED
                break
            rb = _tick(b, snap, resident=True)
            assert ra.records == rb.records and ra.retracts == rb.retracts and ra.redirects == rb.redirects and (ra.new_free == rb.new_free).all()
            a.ready_consume_last(); b.ready_consume_last()
            e.apply(ra)
            # starts, and the retract responses of some Retracting tasks
            for x, tk in sorted(e.tasks.items()):
                if tk.state == core.ASSIGNED and rng.random() < 0.5:
                    e.start_task(x, tk.rv)
            for x, tk in sorted(e.tasks.items()):
                if tk.state == core.RETRACTING and x in e.redirects and rng.random() < 0.4:
                    w = tk.worker
                    e.retract_response(w, [x])
                    assert a.retract_response(w, [x]) == b.retract_response(w, [x])
            # the finish batch: most held tasks by their worker, some by a wrong one, repeats, unknown ids, Retracting ids by their old worker, prefilled ids
            pairs = []
            for x, tk in sorted(e.tasks.items()):
                if tk.state in (core.ASSIGNED, core.RUNNING) and rng.random() < 0.6:
                    pairs.append((x, tk.worker if rng.random() < 0.85 else wids[int(rng.integers(0, len(wids)))]))
                elif tk.state == core.RETRACTING and x in e.redirects and rng.random() < 0.7:
                    pairs.append((x, tk.worker if rng.random() < 0.7 else e.redirects[x][0]))
                elif tk.state == core.PREFILLED and rng.random() < 0.3:
                    pairs.append((x, tk.worker))
            pairs += [pairs[int(rng.integers(0, len(pairs)))] for _ in range(len(pairs) // 5)] if pairs else []
            pairs += [(10**12 + int(rng.integers(0, 50)), wids[0]) for _ in range(2)]
            order = rng.permutation(len(pairs))
            pairs = [pairs[int(k)] for k in order]
            retr_before = {x for x, tk in e.tasks.items() if tk.state == core.RETRACTING}
            got = _finish_checked(a, e, pairs)
            batches += 1
            acc = [p[0] for p, k in zip(pairs, got["kind"].tolist()) if k in ACC]
            # today's sequence on B, for the ids the mirror accepted (a host today has no way to learn that from the library)
            b.assigned_release(acc)
            rel, unknown = b.graph_finish(acc)
            assert unknown == 0 and rel.tolist() == got["released"].tolist()
            for x in acc:  # B's Retracting table has no call that drops a finished task: a response from the old worker erases the entry (the reassignment is ignored)
                if x in retr_before:
                    b.retract_response(e.tasks[x].worker, [x])
            assert a.retracting_count() == b.retracting_count() == sum(1 for tk in e.tasks.values() if tk.state == core.RETRACTING)
            ever = sorted(e.tasks)
            va, vb = (dict(ready=t.ready_count(), sn=t.assigned_count(), pf=t.assigned_prefilled_count(), free=t.assigned_free_rows().tolist(),
                           worker=t.assigned_lookup(ever)[0].tolist(), unf=t.graph_unfinished(ever).tolist()) for t in (a, b))
            assert va == vb
            assert va["unf"] == [0xFFFFFFFF if e.tasks[x].state == core.FINISHED else e.tasks[x].unfinished_deps for x in ever]
            _ledger_matches(a, e)
        assert batches >= 1
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- the call's rules
def _state(t):
    s = t.graph_stats(); s.pop("last_kernel_us", None)
    return dict(ready=t.ready_count(), stats=s)


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
            a.finish_tasks(held, ws)
        assert err.value.code == abi.HQTICK_E_INVALID
        with pytest.raises(HqTickError) as err:
            a.retracting_started([(held[0], ws[0], 0, 0, 0)])
        assert err.value.code == abi.HQTICK_E_INVALID
        a.cluster_upload(e.snapshot())
        cc.seed_ready_graph(a, e)
        before = _state(a)
        with pytest.raises(HqTickError) as err:  # ledger off
            a.finish_tasks(held, ws)
        assert err.value.code == abi.HQTICK_E_INVALID and "assignment ledger not enabled" in str(err.value)
        assert _state(a) == before
        cc.seed_ledger(a, e)
        free = a.assigned_free_rows().copy()
        got = a.finish_tasks([], [])  # n = 0
        assert got["accepted"] == 0 and len(got["kind"]) == 0 and a.assigned_last_unknown() == 0
        import ctypes as C
        a._lib.hqtick_finish_tasks.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p]
        ids = np.asarray(held, np.uint64)
        assert a._lib.hqtick_finish_tasks(a._ctx, 2, ids.ctypes.data_as(abi.u64p), None) == abi.HQTICK_E_INVALID  # a null array
        assert a._lib.hqtick_finish_tasks(a._ctx, 2, None, None) == abi.HQTICK_E_INVALID
        assert a._lib.hqtick_finish_tasks(a._ctx, 0, None, None) == 0
        assert _state(a) == before and (a.assigned_free_rows() == free).all() and a.assigned_count() == 2
        # a two-call tick's placement is pending: refused, nothing changes, and the consume still finds its selection
        res = _tick(a, e.snapshot(), resident=True)
        assert sum(len(r) for r in res.records) == 5
        pending = _state(a)
        with pytest.raises(HqTickError) as err:
            a.finish_tasks(held, ws)
        assert err.value.code == abi.HQTICK_E_INVALID and "pending" in str(err.value)
        assert _state(a) == pending and (a.assigned_free_rows() == free).all() and a.assigned_count() == 2 and a.assigned_lookup(held)[0].tolist() == ws
        a.ready_consume_last()
        e.apply(res)
        assert a.ready_count() == 0 and a.assigned_count() == 7
        got = _finish_checked(a, e, [(held[0], ws[0]), (held[1], ws[0]), (queued[0], e.tasks[queued[0]].worker)])
        assert got["accepted"] == 2 and got["released"].tolist() == [cons] and a.assigned_count() == 5
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- one larger batch
def test_one_larger_batch_against_the_twin():
    """one tick of the 100 000-task x 256-worker workload consumed; every assigned task finished in one call, shuffled, by the right reporters"""
    from hyperqueue_amd.tick import Tick

    snap = workloads.make_steady("c3p", seed=3, n_tasks=100_000, n_workers=256)
    W, R = len(snap.worker_id), snap.n_resources
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    ids, prio, rqs = np.asarray(snap.task_id, np.uint64), np.asarray(snap.task_priority, np.uint64), np.asarray(snap.task_rq, np.uint32)
    cfg = abi.make_config(time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK | abi.HQTICK_FLAG_NO_KERNEL_TIMING)
    a, b = Tick(cfg), Tick(cfg)
    try:
        sc = snap.to_c(resident_workers=True)
        sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None; sc.prefilled_off = None; sc.prefilled_rq = None
        no_deps = (np.zeros(len(ids) + 1, np.uint32), np.zeros(0, np.uint64))
        results = []
        for t in (a, b):
            t.cluster_upload(snap)
            t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
            assert len(t.graph_add_tasks(ids, prio, rqs, no_deps)) == len(ids)
            t.assigned_enable([]); t.assigned_track_prefilled([])
            results.append(abi.parse_result(t.tick_raw(sc, resident=True), W, R))
        res = results[0]
        assert res.records == results[1].records
        wid = snap.worker_id.tolist()
        asg = [(tid, wid[w]) for w, recs in enumerate(res.records) for (tid, v, k) in recs if k == abi.HQ_REC_ASSIGN]
        n_pf = sum(1 for recs in res.records for (tid, v, k) in recs if k == abi.HQ_REC_PREFILL)
        assert len(asg) > 1000 and a.assigned_count() == len(asg) and a.assigned_prefilled_count() == n_pf
        order = np.random.default_rng(11).permutation(len(asg))
        f_ids = np.asarray([asg[k][0] for k in order], np.uint64); f_ws = np.asarray([asg[k][1] for k in order], np.uint32)
        n_ready = a.ready_count()
        got = a.finish_tasks(f_ids, f_ws)
        assert got["accepted"] == len(asg) and (got["kind"] == F.HQ_FINISH_ASSIGNED).all() and len(got["released"]) == 0 and got["graph_unknown"] == 0
        assert a.assigned_count() == 0 and a.assigned_last_unknown() == 0 and a.assigned_prefilled_count() == n_pf and a.ready_count() == n_ready
        total = np.asarray(snap.worker_total, np.uint64).reshape(W, R)
        assert (a.assigned_free_rows() == total).all()  # prefilled tasks hold nothing before they start
        assert b.assigned_release(f_ids) == len(asg)
        rel, unknown = b.graph_finish(f_ids)
        assert unknown == 0 and len(rel) == 0
        assert (a.assigned_free_rows() == b.assigned_free_rows()).all() and b.assigned_count() == 0 and a.ready_count() == b.ready_count()
        sa, sb = a.graph_stats(), b.graph_stats(); sa.pop("last_kernel_us", None); sb.pop("last_kernel_us", None)
        assert sa == sb
        r = a.resident_check(abi.HQ_CHECK_ALL)
        assert r["n_failed"] == 0, r["failed"]
    finally:
        a.close(); b.close()
