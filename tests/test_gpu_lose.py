"""hqtick_lose_workers and its hqtick_lose_last_* accessors (include/hqtick.h) on the device: the reference's lost-worker scenarios through graph +
ready set + ledger with prefilled tracking + the resident Retracting table, every kind in one batch, outputs that do not depend on the order entries sit in the
table, twin contexts (the one call against hqtick_cluster_remove_workers) at batch sizes around the wavefront, tile and padding edges of the sort, gather and
grouping, the merge's three starting states, the call's rules, the batched histories of tests/lose_cases.py, the audit mode and a lost rack."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cancel_cases as cc
import lose_cases as ls
import resident_checks as rc
import start_cases as sc
import test_gpu_finish as gf
import test_gpu_lifecycle as gl
import test_gpu_start as gs
from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

CFG = dict(time_limit_s=20.0)
K = abi
_ctx, _tick, _clean, _prefill_by_hand = gs._ctx, gf._tick, gf._clean, gs._prefill_by_hand


def _answer_matches(got, e, n):
    assert got["n_requeued"] == n == len(e.last_lose_requeued)
    assert got["per_worker"] == e.last_lose_per_worker
    assert got["requeued"] == e.last_lose_requeued
    assert got["reassigned"] == e.last_lose_reassigned
    assert got["mn_left"] == e.last_lose_mn_left
    assert sorted(x[:3] for rows in got["per_worker"] for x in rows) == got["requeued"]  # the union of the lists is the flat list


def _lose_checked(a, e, wids, audit=rc.AUDIT):
    """the batch on the mirror and on context a: the five lists, the older accessors empty, then the whole resident state"""
    mark = len(e.retract_messages)
    n = e.lose_workers(wids)
    got = a.lose_workers(wids)
    print("lost", list(wids), "kinds", [[x[3] for x in rows] for rows in got["per_worker"]], "reassigned", got["reassigned"], "mn_left", got["mn_left"])
    _answer_matches(got, e, n)
    assert a.cluster_last_requeued() == [] and a.cluster_last_requeued_running() == [] and a.cluster_last_requeued_prefilled() == []
    msgs = e.retract_messages[mark:]
    if msgs:  # process_retracted for the prefill sets the requeued tasks dissolved: the host's part, after the call
        rc.DeviceSide(a, "two_call").disposed(e, msgs)
    rc.state_matches(a, e, audit)
    return got


def _kinds(got):
    return {x[0]: x[3] for rows in got["per_worker"] for x in rows}


# ---------------------------------------------------------------------------------------------- 1: the reference's scenarios
def _run_running_task(a):
    e, ws, t1, t2 = sc.scenario_running_task()
    cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
    gs._start_checked(a, e, [(t1, ws[1], 0), (t2, ws[1], 0)])
    got = _lose_checked(a, e, [ws[1]])
    assert _kinds(got) == {t1: K.HQ_LOSE_RUNNING, t2: K.HQ_LOSE_RUNNING}  # test_reactor.rs:562: the client hears [t1, t2]
    return e


def test_running_task():
    a = _ctx()
    try:
        e = _run_running_task(a)
        gf._next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


def test_lost_worker_with_running_and_assign_tasks():
    a = _ctx()
    try:
        e, ws, wf, t1, t2, batch = sc.scenario_lost_worker()
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        gs._start_checked(a, e, batch)
        got = _lose_checked(a, e, [ws[1]])
        assert _kinds(got) == {wf[0]: K.HQ_LOSE_ASSIGNED, wf[1]: K.HQ_LOSE_RUNNING, t1: K.HQ_LOSE_ASSIGNED}  # :590: only wf[1] is reported running
        assert ls.expected_running(e) == [[wf[1]]]
        gf._next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


@pytest.mark.parametrize("who", ["root", "non_root", "both", "both_reversed"])
def test_worker_lost_with_mn_task(who):
    """test_worker_lost_with_mn_task_root (:413-430) and _non_root (:432-449): a three-node task on workers 3, 1, 0 of four"""
    a = _ctx()
    try:
        e, t1, root, other = sc.scenario_mn_root()
        cc.seed_ledger(a, e); a.assigned_track_prefilled([]); cc.seed_ready_graph(a, e)
        spare = e.new_worker(WB(1)); s = e.snapshot()  # (a fifth worker, so that two may go)
        tot = np.asarray(s.worker_total, np.uint64).reshape(len(s.worker_id), s.n_resources)[s.worker_id.tolist().index(spare)][None, :]
        a.cluster_add_workers([spare], tot, tot)
        lost = {"root": [root], "non_root": [other], "both": [root, other], "both_reversed": [other, root]}[who]
        got = _lose_checked(a, e, lost)
        if who == "non_root":
            assert got["mn_left"] == [(t1, other, root)] and got["n_requeued"] == 0 and e.tasks[t1].state == core.RUNNING_MN and a.assigned_mn_count() == 1
            assert a.assigned_mn_workers(t1)[0] == root and other not in a.assigned_mn_workers(t1)
        else:
            assert _kinds(got) == {t1: K.HQ_LOSE_MN_ROOT} and got["mn_left"] == [] and e.tasks[t1].state == core.WAITING and a.assigned_mn_count() == 0
            assert got["per_worker"][lost.index(root)] == [(t1, e.tasks[t1].rq, e.tasks[t1].priority, K.HQ_LOSE_MN_ROOT)]
            assert all(f & abi.HQ_WORKER_SN for f in a.cluster_worker_flags().tolist())  # the other nodes are free single-node workers again
    finally:
        a.close()


def test_lost_worker_with_a_prefilled_task():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e = SchedEnv(abi.make_config(reserve=1, fill_max=1, **CFG))
        tasks = e.new_tasks(3, TB())
        w1 = e.new_worker(WB(1)); others = [e.new_worker(WB(1)) for _ in range(3)]
        for w in others:  # (busy, so that the tick fills w1 only)
            e.new_task_assigned(TB(), w)
        snap = e.snapshot()
        a.cluster_upload(snap)
        held = [x for x in e.tasks.values() if x.state == core.ASSIGNED]
        a.assigned_enable([(x.id, x.worker, x.rq, x.rv, x.priority) for x in held]); a.assigned_track_prefilled([])
        e.apply(_tick(a, snap))
        cc.seed_ready_graph(a, e)
        prefilled = next(x for x in tasks if e.task(x).is_prefilled())
        w = e.tasks[prefilled].worker  # (w1 in the reference's scenario: the one worker with room)
        want = {x: K.HQ_LOSE_ASSIGNED for x in e.workers[w].assigned_tasks}
        want.update({x: K.HQ_LOSE_PREFILLED for x in e.workers[w].prefilled_tasks})
        n_pf = a.assigned_prefilled_count()
        got = _lose_checked(a, e, [w])
        assert _kinds(got) == want and K.HQ_LOSE_ASSIGNED in want.values() and a.assigned_prefilled_count() == n_pf - sum(k == K.HQ_LOSE_PREFILLED for k in want.values())
        assert e.tasks[prefilled].state == core.WAITING and prefilled in e.ready[e.tasks[prefilled].rq]
    finally:
        a.close()


@pytest.mark.parametrize("who", ["old", "target", "both", "both_reversed"])
def test_lost_worker_of_a_retracting_task(who):
    """setup_retracting (test_reactor.rs:993-1007): t is Retracting{w1} with a redirect to w2.  w1 lost: Assigned on w2, one ComputeTasks message (reactor.rs:131-141);
    w2 lost: the redirect is dropped, t is back in its queue and still Retracting{w1} (:90-96); both: Waiting, no message"""
    a = _ctx(reserve=1, fill_max=1)
    try:
        e, w1, w2, t, others = gf._retracting_pair(a)
        more = [e.new_worker(WB(1)) for _ in range(3)]; s = e.snapshot()
        tot = np.asarray(s.worker_total, np.uint64).reshape(len(s.worker_id), s.n_resources)[[s.worker_id.tolist().index(w) for w in more]]
        a.cluster_add_workers(more, tot, tot)
        cc.seed_ready_graph(a, e)
        v = e.redirects[t][1]
        got = _lose_checked(a, e, {"old": [w1], "target": [w2], "both": [w1, w2], "both_reversed": [w2, w1]}[who])
        x = e.tasks[t]
        if who == "old":
            assert got["reassigned"] == [(t, w2, v)] and x.state == core.ASSIGNED and x.worker == w2 and t not in _kinds(got) and a.retracting_count() == 0
        elif who == "target":
            assert got["reassigned"] == [] and _kinds(got)[t] == K.HQ_LOSE_REDIRECT and x.state == core.RETRACTING and x.worker == w1 and a.retracting_count() == 1
            assert a.assigned_lookup([t])[0].tolist() == [abi.HQ_NO_WORKER]
        else:
            assert got["reassigned"] == [] and _kinds(got)[t] == K.HQ_LOSE_REDIRECT and x.state == core.WAITING and a.retracting_count() == 0
        gf._next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 2: every kind in one batch
def _all_kinds_env(a):
    """gf._kinds_env's five workers (w1 holds an assigned task and is what t_red retracts FROM, w2 is t_red's redirect target, w3 holds three plain tasks -- one
    reported running here --, a prefilled one and is what t_q retracts from, root and node run a two-node task) and three more: a second two-node task on wa (root)
    and wb, and wc that holds nothing; 30 more waiting tasks on both sides of the held ids"""
    e, ws, t = gf._kinds_env(a, None)
    w1, w2, w3, root, node = ws
    more = [e.new_worker(WB(4)) for _ in range(3)]; s = e.snapshot()
    tot = np.asarray(s.worker_total, np.uint64).reshape(len(s.worker_id), s.n_resources)[[s.worker_id.tolist().index(w) for w in more]]
    a.cluster_add_workers(more, tot, tot)
    wa, wb, wc = more
    mn2 = e.new_task(TB().n_nodes(2))
    extra = [e.new_task(TB().cpus(1)) for _ in range(30)]  # (no tick comes before the loss: they wait)
    e.ready[e.tasks[mn2].rq].discard(mn2)
    e.start_task_mn(mn2, [wa, wb])
    x = e.tasks[mn2]
    new = [mn2] + extra
    a.graph_add_tasks(new, [e.tasks[y].priority for y in new], [e.tasks[y].rq for y in new], [[] for _ in new])
    assert a.ready_remove([mn2]) == 1
    assert a.assigned_add_mn([(mn2, x.rq, x.priority, [wa, wb])]) == 1
    gs._start_checked(a, e, [(t["sn"][2], w3, 0)])
    rc.state_matches(a, e)
    return e, dict(w1=w1, w2=w2, w3=w3, root=root, node=node, wa=wa, wb=wb, wc=wc), dict(t, mn2=mn2)


def test_every_kind_in_one_batch():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e, w, t = _all_kinds_env(a)
        assert len(e.workers) == 8 and len(e.tasks) >= 40
        lost = [w["wb"], w["w3"], w["wc"], w["root"], w["w2"]]  # (neither ascending nor descending)
        sn = t["sn"]
        on_w2 = sorted(x for x in e.workers[w["w2"]].assigned_tasks if x != t["red"])
        got = _lose_checked(a, e, lost)
        want = {sn[0]: K.HQ_LOSE_ASSIGNED, sn[1]: K.HQ_LOSE_ASSIGNED, sn[2]: K.HQ_LOSE_RUNNING, t["pf"]: K.HQ_LOSE_PREFILLED, t["mn"]: K.HQ_LOSE_MN_ROOT, t["red"]: K.HQ_LOSE_REDIRECT}
        want.update({x: K.HQ_LOSE_ASSIGNED for x in on_w2})
        assert _kinds(got) == want and set(want.values()) == set(range(5))
        assert [[x[0] for x in rows] for rows in got["per_worker"]] == [[], sorted(sn + [t["pf"]]), [], [t["mn"]], sorted(on_w2 + [t["red"]])]
        assert got["mn_left"] == [(t["mn2"], w["wb"], w["wa"])] and got["reassigned"] == []
        assert e.tasks[t["red"]].state == core.RETRACTING and e.tasks[t["q"]].state == core.WAITING and a.retracting_count() == 1  # (t_q was retracting from w3)
        assert sorted(e.workers) == sorted([w["w1"], w["node"], w["wa"]]) and a.assigned_mn_workers(t["mn2"]) == [w["wa"]]
        gf._ready_is(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 3: the order of the outputs
def _rack_env(n_lost, k, n_stay=3, mn=False, seed=0):
    """n_lost + n_stay workers of 1024 cpus; k one-cpu tasks on the lost ones (dealt round-robin in a shuffled order: ids interleave across workers), of which every
    fifth is prefilled and every third of the others will be reported running; 7 more on the staying workers; 5 waiting tasks with ids below and 5 with ids above
    -> (mirror, lost workers, staying workers, the start batch)"""
    rng = np.random.default_rng([n_lost, k, seed])
    e = SchedEnv(abi.make_config(**CFG))
    ws = e.new_workers_cpus([1024] * (n_lost + n_stay))
    lost = [ws[int(j)] for j in sorted(rng.choice(len(ws), n_lost, replace=False))]
    stay = [w for w in ws if w not in lost]
    e.new_tasks(5, TB())
    held = e.new_tasks(k, TB())
    start = []
    for j, x in enumerate(held):
        w = lost[int(rng.integers(0, n_lost))] if j >= n_lost else lost[j]  # (every lost worker holds one where k allows)
        if j % 5 == 3:
            _prefill_by_hand(e, x, w)
        else:
            e.assign_task(x, w)
            if j % 3 == 1:
                start.append((x, w, 0))
    for j, x in enumerate(e.new_tasks(7, TB())):
        e.assign_task(x, stay[j % n_stay])
    e.new_tasks(5, TB())
    return e, lost, stay, start


def _seed(a, e, start):
    cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
    if start:
        assert a.start_tasks(*gs._cols(e, start))["accepted"] == len(start)


def test_order_not_by_arrival():
    """the same logical state on two contexts whose tables differ in capacity, insert order and tombstones: b's ledger is enabled with the entries in another
    order, then grown past its first table by 900 entries on a ninth worker (a rebuild re-inserts the live entries), which then is removed (900 tombstones)"""
    a, b = _ctx(), _ctx()
    try:
        e, lost, stay, start = _rack_env(4, 300)
        _seed(a, e, [])
        snap = e.snapshot()
        ghost = max(e.workers) + 7
        e2 = SchedEnv(abi.make_config(**CFG))  # (the same workers plus the ninth, for b's upload)
        for _ in e.workers:
            e2.new_worker(WB(1024))
        assert sorted(e2.workers) == sorted(e.workers)
        e2.worker_id_counter = ghost; assert e2.new_worker(WB(1024)) == ghost
        e2.rq_id(TB())
        s2 = e2.snapshot()
        b.cluster_upload(s2)
        live = [x for x in cc.live_tasks(e) if x.state in (core.ASSIGNED, core.RUNNING)]
        order = np.random.default_rng(3).permutation(len(live))
        b.assigned_enable([(live[j].id, live[j].worker, live[j].rq, live[j].rv, live[j].priority) for j in order])
        pf = [(x.id, x.worker, x.rq, x.priority) for x in cc.live_tasks(e) if x.state == core.PREFILLED][::-1]
        assert b.assigned_track_prefilled(pf) == len(pf)
        dummy = list(range(10**6, 10**6 + 900))
        assert b.assigned_add([(x, ghost, 0, 0, 0) for x in dummy]) == 900
        assert b.cluster_remove_workers([ghost]) == [] and len(b.cluster_last_requeued()) == 900  # (no ready set yet: only reported)
        free = cc.free_rows(e)
        b.cluster_update_workers(list(range(len(e.workers))), free)  # (the rows as the mirror has them: b's upload knew the workers as idle)
        cc.seed_ready_graph(b, e)
        for c in (a, b):
            assert c.start_tasks(*gs._cols(e, start))["accepted"] == len(start)
        e.start_tasks(start)
        rc.state_matches(a, e); rc.state_matches(b, e)
        batch = [lost[2], lost[0], lost[3], lost[1]]
        n = e.lose_workers(batch)
        ga, gb = a.lose_workers(batch), b.lose_workers(batch)
        assert ga == gb
        _answer_matches(ga, e, n)
        assert n == 300 and set(_kinds(ga).values()) == {K.HQ_LOSE_ASSIGNED, K.HQ_LOSE_RUNNING, K.HQ_LOSE_PREFILLED}
        rc.state_matches(a, e); rc.state_matches(b, e)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 4: batch sizes, against the parent's call
SIZES = [(k, n) for k in (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513) for n in (1, 2, 64, 65) if n <= k]


@pytest.mark.parametrize("k,n", SIZES)
def test_batch_sizes_against_the_parents_call(k, n):
    """k evicted entries (the wavefront, slice and power-of-two-padding edges of the eviction's append, the sort, the gather and the grouping) of n lost workers,
    wherever every lost worker can hold one: the same state on two contexts, one taking hqtick_cluster_remove_workers and one hqtick_lose_workers"""
    a, b = _ctx(), _ctx()
    try:
        e, lost, stay, start = _rack_env(n, k)
        _seed(a, e, start); _seed(b, e, start)
        e.start_tasks(start)
        ids = sorted(e.tasks)
        batch = [lost[int(j)] for j in np.random.default_rng([k, n]).permutation(n)]
        n_req = e.lose_workers(batch)
        got = a.lose_workers(batch)
        sent = b.cluster_remove_workers(batch)
        assert n_req == k
        _answer_matches(got, e, n_req)
        assert got["reassigned"] == sent == []
        assert rc.digest(a, ids) == rc.digest(b, ids)
        rc.state_matches(a, e); rc.state_matches(b, e)
        assert got["requeued"] == b.cluster_last_requeued()
        kinds = _kinds(got)
        assert b.cluster_last_requeued_running() == sorted(x for x, kd in kinds.items() if kd in abi.HQ_LOSE_RUNNING_TASKS) == sorted(x[0] for x in start)
        assert b.cluster_last_requeued_prefilled() == sorted(x for x, kd in kinds.items() if kd == K.HQ_LOSE_PREFILLED)
        gf._ready_is(a, e)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 5: the merge's three starting states
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("ready", ["nothing", "tombstones", "both_sides"])
def test_the_merge_from_every_starting_state(ready, shuffled):
    a = _ctx()
    try:
        e, lost, stay, start = _rack_env(3, 70)
        waiting = sorted(x for s in e.ready.values() for x in s)
        if ready != "both_sides":  # the waiting tasks are cancelled: before the upload, or out of the resident set (their rows stay behind as tombstones)
            if ready == "nothing":
                e.cancel_tasks(waiting)
        _seed(a, e, start)
        e.start_tasks(start)
        if ready == "tombstones":
            e.cancel_tasks(waiting)
            a.cancel_tasks(waiting)
            assert a.ready_count() == 0
        rc.state_matches(a, e)
        batch = [lost[k] for k in ((2, 0, 1) if shuffled else (0, 1, 2))]
        got = _lose_checked(a, e, batch)
        assert got["n_requeued"] == 70 and a.ready_count() == 70 + (10 if ready == "both_sides" else 0)
        gf._ready_is(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 6: the call's rules
def test_call_rules():
    from hyperqueue_amd.tick import HqTickError

    def refused(call, text=None):
        with pytest.raises(HqTickError) as err:
            call()
        assert err.value.code == abi.HQTICK_E_INVALID and (text is None or text in str(err.value)), str(err.value)

    a = _ctx()
    try:
        e, lost, stay, start = _rack_env(2, 9)
        refused(lambda: a.lose_workers([lost[0]]), "without hqtick_cluster_upload")  # no worker set
        a.cluster_upload(e.snapshot())
        refused(lambda: a.lose_workers([lost[0]]), "no resident ready set")
        a.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        refused(lambda: a.lose_workers([lost[0]]), "assignment ledger not enabled")
        assert a.cluster_workers().tolist() == sorted(e.workers)
        _seed(a, e, start)
        e.start_tasks(start)
        ids = sorted(e.tasks)
        before = rc.digest(a, ids)
        refused(lambda: a.lose_workers([max(e.workers) + 1]), "unknown (or repeated) worker id")
        refused(lambda: a.lose_workers([lost[0], stay[0], lost[0]]), "unknown (or repeated) worker id")
        f = a._lib.hqtick_lose_workers
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u32p]
        assert f(a._ctx, 2, None) == abi.HQTICK_E_INVALID  # a null array
        assert rc.digest(a, ids) == before
        got = a.lose_workers([])  # n = 0: every list empty
        assert got == dict(n_requeued=0, per_worker=[], requeued=[], reassigned=[], mn_left=[]) and rc.digest(a, ids) == before
        # a two-call tick's placement is pending: refused, nothing changes, and the consume still finds its selection
        res = _tick(a, e.snapshot(), resident=True)
        assert sum(len(r) for r in res.records) > 0
        before = rc.digest(a, ids)
        rc.expect_pending(lambda: a.lose_workers([lost[0]]))
        assert rc.digest(a, ids) == before
        a.ready_consume_last(); e.apply(res)
        rc.state_matches(a, e)
        # the lists live until the next hqtick_lose_workers: a hqtick_cluster_remove_workers behind the call answers through its own accessors and leaves them
        got = _lose_checked(a, e, [lost[1]])
        assert got["n_requeued"] > 0
        held = sorted(e.workers[lost[0]].assigned_tasks | e.workers[lost[0]].prefilled_tasks)
        sent = e.remove_worker(lost[0])
        assert a.cluster_remove_workers([lost[0]]) == sent
        assert [x[0] for x in a.cluster_last_requeued()] == held and held
        assert a.lose_last() == {k: v for k, v in got.items() if k != "n_requeued"}
        rc.state_matches(a, e)
        got = a.lose_workers([])  # ... and an empty call empties them
        assert got["per_worker"] == [] and got["requeued"] == [] and [x[0] for x in a.cluster_last_requeued()] == held
    finally:
        a.close()


def test_a_refused_merge_leaves_the_lists_filled():
    """the last step fails -- the host had put an id into the ready set that a lost worker still held, and the merge refuses the duplicate: the call returns the
    error, the workers, the entries and the Retracting table have moved, the ready set is as it was, and the five lists are there for the host to finish with"""
    from hyperqueue_amd.tick import HqTickError

    a = _ctx()
    try:
        e, lost, stay, start = _rack_env(2, 9)
        _seed(a, e, start)
        e.start_tasks(start)
        stray = min(e.workers[lost[0]].assigned_tasks)
        a.ready_add([stray], [e.tasks[stray].priority], [e.tasks[stray].rq])  # (the host's mistake)
        n_ready = a.ready_count()
        n = e.lose_workers(lost)
        with pytest.raises(HqTickError) as err:
            a.lose_workers(lost)
        assert err.value.code == abi.HQTICK_E_INVALID and "already in the ready set" in str(err.value), str(err.value)
        got = a.lose_last()
        _answer_matches(dict(got, n_requeued=n), e, n)
        assert n == 9 and a.ready_count() == n_ready and a.cluster_workers().tolist() == sorted(e.workers)
        # the host takes its stray id back and adds what the call reported: the state is the mirror's
        assert a.ready_remove([stray]) == 1
        a.ready_add([x[0] for x in got["requeued"]], [x[2] for x in got["requeued"]], [x[1] for x in got["requeued"]])
        rc.state_matches(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 7: the histories, the audit mode
class Dev(rc.DeviceSide):
    """resident_checks.DeviceSide whose lost workers go through hqtick_lose_workers, a batch at a time"""

    def lose(self, e, wids, info):
        a = self.a
        got = a.lose_workers(wids)
        _answer_matches(got, e, info["n"])
        back = {x for s in e.ready.values() for x in s} - info["ready_before"] - set(info["disposed"])
        assert [x[0] for x in got["requeued"]] == sorted(back)
        assert a.cluster_last_requeued() == [] and a.cluster_last_requeued_running() == []


def _play(form, seed):
    oracle = Oracle(abi.make_config(reserve=1, fill_max=2, **ls.lc.CFG), canonical=True)
    a = gl._ctx(form, reserve=1, fill_max=2)
    try:
        given = lambda: Oracle(abi.make_config(reserve=1, fill_max=2, **ls.lc.CFG))
        return ls.play(ls.history(seed, form), oracle, Dev(a, form, given))
    finally:
        a.close()


@pytest.mark.parametrize("form,seed", [(form, seed) for form in ls.FORMS for seed in ls.SEEDS[form]])
def test_history(form, seed):
    h = _play(form, seed)
    print(f"{form} seed {seed}: {len(h.log)} steps, {h.rounds_done} rounds, " + " ".join(f"{k}={v}" for k, v in sorted(h.cov.items()) if k in ls.LINES))


def test_audit_mode_runs_a_history():
    """a context created with HQTICK_CHECK_RESIDENT=1 audits itself after every call that changes resident state, hqtick_lose_workers among them: the first history
    runs through (a child process: the variable is read when the library creates the context)"""
    here = os.path.dirname(os.path.abspath(__file__))
    form = ls.FORMS[0]
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_lose as g\n"
            "h = g._play(%r, %d)\nprint('AUDITED-OK', len(h.log))\n") % (os.path.dirname(here), here, form, ls.SEEDS[form][0])
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HQTICK_CHECK_RESIDENT="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "AUDITED-OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- 8: a lost rack
def test_lost_rack_and_placed_again():
    """64 workers of 128 cpus, 3 500 tasks placed by one tick; every second worker is lost in one call: half of the entries go back, and the next tick's
    placement is the oracle's on the mirror"""
    cfg = abi.make_config(**CFG)
    a = _ctx()
    try:
        e = SchedEnv(cfg)
        ws = [e.new_worker(WB(128)) for _ in range(64)]
        for k in range(3500):
            e.new_task(TB().cpus(2) if k % 7 == 0 else TB().cpus(1))
        snap = e.snapshot()
        a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
        e.apply(_tick(a, snap))
        assert a.assigned_count() == 3500
        cc.seed_ready_graph(a, e)
        lost = [ws[int(j)] for j in np.random.default_rng(8).permutation(64)[:32]]
        n = e.lose_workers(lost)
        got = a.lose_workers(lost)
        _answer_matches(got, e, n)
        assert 1000 < n < 2500 and a.assigned_count() == 3500 - n and a.ready_count() == n
        rc.ledger_matches(a, e)
        assert (a.assigned_free_rows() == cc.free_rows(e)).all() and a.cluster_workers().tolist() == sorted(e.workers)
        _clean(a)
        dev = rc.DeviceSide(a, "two_call", lambda: Oracle(cfg))
        snap = e.snapshot()
        want, code = ls.lc.oracle_tick(Oracle(cfg, canonical=True), snap)
        want = dev.tick(e, snap, want, code)
        assert sum(len(r) for r in want.records) == n
        a.ready_consume_last(); e.apply(want)
        rc.ledger_matches(a, e)
        assert (a.assigned_free_rows() == cc.free_rows(e)).all() and a.ready_count() == 0
    finally:
        a.close()
