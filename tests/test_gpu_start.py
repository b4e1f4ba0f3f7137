"""hqtick_start_tasks, hqtick_assigned_running and hqtick_cluster_last_requeued_running (include/hqtick.h) on the device: the reference's
task_running / on_remove_worker scenarios through graph + ready set + ledger with prefilled tracking + the resident Retracting table, every kind in one batch,
the claim decided by position at wave and workgroup edges, twin contexts (the one call against hqtick_assigned_start_prefilled + hqtick_retracting_started driven
by the mirror's states) at batch sizes around those edges, the claim words given back, the running byte across a table rebuild and a re-pack, the batch order
under saturating arithmetic, the call's rules, the audit mode and one larger batch."""
import copy
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import cancel_cases as cc
import resident_checks as rc
import start_cases as sc
import test_gpu_finish as gf
from hyperqueue_amd import abi, core, workloads
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

pytestmark = pytest.mark.gpu

AUDIT = abi.HQ_CHECK_ALL | abi.HQ_CHECK_STRICT
CFG = dict(time_limit_s=20.0)
ACC = abi.HQ_START_ACCEPTED
K = abi
NO_ENTRY = 0xFF
_clean, _tick = gf._clean, gf._tick


def _ctx(**kw):
    from hyperqueue_amd.tick import Tick

    return Tick(abi.make_config(**{**CFG, **kw}))


def _cols(e, triples):
    """the five columns of the call: ids, reporters, variants and the tasks' own request and priority (0 for an id the mirror does not know)"""
    ids = [t[0] for t in triples]
    return (ids, [t[1] for t in triples], [t[2] for t in triples], [e.tasks[x].rq if x in e.tasks else 0 for x in ids],
            [e.tasks[x].priority if x in e.tasks else 0 for x in ids])


_running_want, _entries_match = rc.running_want, rc.entries_match  # (the comparison itself: tests/resident_checks.py)


def _start_checked(a, e, triples, overfull=False):
    """the batch on the mirror and on context a, the audit clean before and after: kinds, accepted and refused counts, ready count, free rows, ledger counts,
    running bytes and variants must agree.  overfull: the batch over-commits a worker as start_prefilled may (saturating free.remove, workerload.rs:156-165):
    HQ_INV_LEDGER_FREE may speak afterwards, and only that"""
    _clean(a)
    want = e.start_tasks(triples)
    kinds = e.last_start_kinds
    got = a.start_tasks(*_cols(e, triples))
    print("kinds", got["kind"].tolist(), "accepted", got["accepted"])
    assert got["kind"].tolist() == kinds
    assert got["accepted"] == want == sum(k in ACC for k in kinds) and a.assigned_last_unknown() == len(triples) - want
    assert a.ready_count() == gf._ready_total(e)
    assert (a.assigned_free_rows() == cc.free_rows(e)).all()
    assert a.retracting_count() == sum(1 for t in e.tasks.values() if t.state == core.RETRACTING)
    gf._ledger_matches(a, e)
    _entries_match(a, e)
    if overfull:
        assert set(a.resident_check(AUDIT)["failed"]) <= {"HQ_INV_LEDGER_FREE"}
    else:
        _clean(a)
    return got


def _lose_worker(a, e, wid):
    """on_remove_worker on both sides: the running list, the requeued ids and the ready count agree"""
    before = {x for s in e.ready.values() for x in s}
    sent = e.remove_worker(wid)
    assert a.cluster_remove_workers([wid]) == sent
    assert a.cluster_last_requeued_running() == e.last_lost_running
    requeued = [x[0] for x in a.cluster_last_requeued()]
    assert set(requeued) == {x for s in e.ready.values() for x in s} - before and set(e.last_lost_running) <= set(requeued)
    assert a.ready_count() == gf._ready_total(e)
    _clean(a)


# ---------------------------------------------------------------------------------------------- 1: the reference's scenarios
def _run_running_task(a):
    e, ws, t1, t2 = sc.scenario_running_task()
    cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
    assert a.assigned_running([t1, t2, 10**12]).tolist() == [0, 0, NO_ENTRY]
    assert _start_checked(a, e, [(t1, ws[1], 0)])["kind"].tolist() == [K.HQ_START_ASSIGNED]
    assert _start_checked(a, e, [(t2, ws[1], 0)])["kind"].tolist() == [K.HQ_START_ASSIGNED]
    sc.check_running_task(e, ws, t1, t2)
    got = _start_checked(a, e, [(t1, ws[0], 0), (t1, ws[1], 1), (t1, ws[1], 0), (10**12, ws[1], 0)])
    assert got["kind"].tolist() == [K.HQ_START_WRONG_WORKER, K.HQ_START_WRONG_VARIANT, K.HQ_START_RUNNING, K.HQ_START_NONE]
    _lose_worker(a, e, ws[1])
    assert a.cluster_last_requeued_running() == [t1, t2]  # test_reactor.rs:562
    return e


def test_running_task():
    a = _ctx()
    try:
        e = _run_running_task(a)
        gf._next_tick_equals_the_mirrors(a, e)
        assert 1 not in a.assigned_running(sorted(e.tasks)).tolist()  # the requeued tasks the tick placed again are not running yet
    finally:
        a.close()


def test_lost_worker_with_running_and_assign_tasks():
    a = _ctx()
    try:
        e, ws, wf, t1, t2, batch = sc.scenario_lost_worker()
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        assert _start_checked(a, e, batch)["kind"].tolist() == [K.HQ_START_ASSIGNED]
        _lose_worker(a, e, ws[1])
        sc.check_lost_worker(e, ws, wf, t1, t2)
        assert a.cluster_last_requeued_running() == [wf[1]]  # :590: the merely assigned wf[0] and t1 are requeued, not reported
        assert sorted(x[0] for x in a.cluster_last_requeued()) == sorted([wf[0], wf[1], t1])
        gf._next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


def test_prefill_started():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e = SchedEnv(abi.make_config(reserve=1, fill_max=1, **CFG))
        tasks = e.new_tasks(3, TB())
        w1 = e.new_worker(WB(1))
        snap = e.snapshot()
        a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
        e.apply(_tick(a, snap))
        assigned = next(x for x in tasks if e.task(x).is_assigned()); prefilled = next(x for x in tasks if e.task(x).is_prefilled())
        cc.seed_ready_graph(a, e)
        assert a.assigned_running([assigned, prefilled]).tolist() == [0, 0]  # entered by a tick, as an assignment and as a prefill
        gf._finish_checked(a, e, [(assigned, w1)])
        got = _start_checked(a, e, [(prefilled, w1 + 1, 0), (prefilled, w1, 5), (prefilled, w1, 0), (prefilled, w1, 0)])
        assert got["kind"].tolist() == [K.HQ_START_WRONG_WORKER, K.HQ_START_BAD_VARIANT, K.HQ_START_PREFILLED, K.HQ_START_REPEAT]
        assert a.assigned_prefilled_count() == 0 and a.assigned_count() == 1 and a.assigned_running([prefilled]).tolist() == [1]
        x = e.tasks[prefilled]
        assert x.state == core.RUNNING and x.worker == w1 and not e.workers[w1].prefilled_tasks
    finally:
        a.close()


def test_prefill_started_on_same_worker():
    a = _ctx(reserve=0, fill_max=3)
    try:
        e = SchedEnv(abi.make_config(reserve=0, fill_max=3, **CFG))
        state = {"first": True}

        def schedule():
            snap = e.snapshot()
            if state["first"]:
                a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
                state["first"] = False
            e.apply(_tick(a, snap))

        w1, t1, assigned, prefilled = sc.setup_same_worker(e, schedule)
        e.new_task(TB().cpus(3))  # fits no worker: the tick below needs a ready task
        e.finish_tasks([(t1, w1)])
        assert a.assigned_release([t1]) == 1
        schedule()
        assert e.task(prefilled).is_retracting() and a.retracting_count() == 1  # test_reactor.rs:897
        assert a.assigned_lookup([prefilled])[1].tolist() == [0] and a.assigned_prefilled_count() == 0  # the tick's upsert made the prefilled entry an assigned one
        cc.seed_ready_graph(a, e)
        got = _start_checked(a, e, [(prefilled, w1, 0)])
        assert got["kind"].tolist() == [K.HQ_START_RETRACTING]
        sc.check_same_worker(e, w1, prefilled)
        assert a.assigned_lookup([prefilled])[0].tolist() == [w1] and a.assigned_running([prefilled]).tolist() == [1]
    finally:
        a.close()


def test_steal_running():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e, w1, w2, t, others = gf._retracting_pair(a)
        cc.seed_ready_graph(a, e)
        assert a.assigned_running([t]).tolist() == [0]  # the redirect's entry, entered by the tick's upsert
        (on_w1,) = sorted(e.workers[w1].assigned_tasks)
        gf._finish_checked(a, e, [(on_w1, w1)])
        got = _start_checked(a, e, [(t, w2, 0)])  # the redirect TARGET never got the task: refused, nothing changes
        assert got["kind"].tolist() == [K.HQ_START_WRONG_WORKER] and a.retracting_count() == 1 and a.assigned_lookup([t])[0].tolist() == [w2]
        got = _start_checked(a, e, [(t, w1, 0), (t, w1, 0), (t, w2, 0)])
        assert got["kind"].tolist() == [K.HQ_START_RETRACTING, K.HQ_START_REPEAT, K.HQ_START_WRONG_WORKER]
        sc.check_steal_running(e, w1, w2, t, on_w1)
        assert a.retracting_count() == 0 and a.assigned_lookup([t])[0].tolist() == [w1] and a.assigned_running([t]).tolist() == [1]
        gf._next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


def test_a_retracting_tasks_entry_on_a_lost_target_is_not_running():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e, w1, w2, t, others = gf._retracting_pair(a)
        cc.seed_ready_graph(a, e)
        (on_w2,) = [x for x in e.workers[w2].assigned_tasks if x != t]
        _start_checked(a, e, [(on_w2, w2, e.tasks[on_w2].rv)])
        _lose_worker(a, e, w2)
        assert a.cluster_last_requeued_running() == [on_w2] and e.tasks[t].is_retracting()
    finally:
        a.close()


def test_worker_lost_with_mn_task_root():
    a = _ctx()
    try:
        e, t1, root, other = sc.scenario_mn_root()
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        got = _start_checked(a, e, [(t1, root, 0), (t1, other, 0), (t1, root, 0)])
        assert got["kind"].tolist() == [K.HQ_START_MN, K.HQ_START_WRONG_WORKER, K.HQ_START_MN] and got["accepted"] == 2
        assert a.assigned_running([t1]).tolist() == [0]  # its class says it runs
        _lose_worker(a, e, root)
        assert a.cluster_last_requeued_running() == [t1] and e.tasks[t1].state == core.WAITING and a.assigned_mn_count() == 0
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 2: every kind in one batch
def _kinds_batch(e, ws, t):
    w1, w2, w3, root, node = ws
    sn = t["sn"]
    triples = [(sn[0], root, 0), (sn[0], w3, 1), (sn[0], w3, 0), (sn[0], w3, 0), (sn[2], w3, 0), (t["red"], w2, 0), (t["red"], w1, 9), (t["red"], w1, 0), (t["red"], w1, 0),
               (10**12, w1, 0), (t["pf"], w3, 7), (t["pf"], w3, 0), (t["pf"], w3, 0), (t["q"], w3, 0), (t["waiting"], w3, 0), (t["mn"], root, 0), (t["mn"], node, 0),
               (t["mn"], root, 0), (t["q"], w3, 0)]
    want = [K.HQ_START_WRONG_WORKER, K.HQ_START_WRONG_VARIANT, K.HQ_START_ASSIGNED, K.HQ_START_REPEAT, K.HQ_START_RUNNING, K.HQ_START_WRONG_WORKER, K.HQ_START_BAD_VARIANT,
            K.HQ_START_RETRACTING, K.HQ_START_REPEAT, K.HQ_START_NONE, K.HQ_START_BAD_VARIANT, K.HQ_START_PREFILLED, K.HQ_START_REPEAT, K.HQ_START_RETRACTING, K.HQ_START_NONE,
            K.HQ_START_MN, K.HQ_START_WRONG_WORKER, K.HQ_START_MN, K.HQ_START_REPEAT]
    return triples, want


def test_every_kind_in_one_batch():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e, ws, t = gf._kinds_env(a, None)
        _entries_match(a, e)  # entered by ticks, an upsert (the redirect), a seed, by hand: nothing runs yet
        assert 1 not in a.assigned_running(sorted(e.tasks)).tolist()
        (on_w1,) = sorted(e.workers[ws[0]].assigned_tasks)
        gf._finish_checked(a, e, [(t["sn"][1], ws[2]), (on_w1, ws[0])])  # (room on w3 and w1 for the prefilled and the Retracting tasks that start there)
        _start_checked(a, e, [(t["sn"][2], ws[2], 0)])
        triples, want = _kinds_batch(e, ws, t)
        n_ready = a.ready_count()
        got = _start_checked(a, e, triples)
        assert got["kind"].tolist() == want and set(want) == set(range(10))
        assert got["accepted"] == 6 and a.retracting_count() == 0 and a.assigned_prefilled_count() == 0
        assert a.ready_count() == n_ready - 1  # the in-queue Retracting id left its queue
        assert a.assigned_lookup([t["red"], t["q"], t["pf"]])[0].tolist() == [ws[0], ws[2], ws[2]]
        assert a.assigned_running([t["red"], t["q"], t["pf"], t["sn"][0], t["sn"][2], t["mn"], t["waiting"]]).tolist() == [1, 1, 1, 1, 1, 0, NO_ENTRY]
        gf._ready_is(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 3: the claim goes to the lower position
def _prefill_by_hand(e, x, wid):
    """task x (in its queue) becomes Prefilled on worker wid in the mirror, as a tick's prefill leaves it"""
    y = e.tasks[x]
    y.state, y.worker = core.PREFILLED, wid
    e.workers[wid].prefilled_tasks.add(x); e.ready[y.rq].discard(x)
    if y.rq not in e.prefill:
        e.prefill[y.rq] = (y.priority, core.task_id_set())
    e.prefill[y.rq][1].insert(x)


def test_claim_by_position_not_by_arrival():
    """two positions of one prefilled id with different valid variants, at both sides of a wavefront and a workgroup edge and in two workgroups, in both orders: the
    lower position's variant is the entry's, the other position is a repeat"""
    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        (w,) = e.new_workers_cpus([64])
        two = TB().cpus(2).next_variant().cpus(1)
        cases = [(p, q, first) for (p, q) in ((0, 1), (63, 64), (255, 256), (0, 256)) for first in (0, 1)]
        pf = [e.new_task(two) for _ in cases]
        for x in pf:
            _prefill_by_hand(e, x, w)
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        for x, (p, q, first) in zip(pf, cases):
            triples = [(10**12 + k, w, 0) for k in range(257)]
            triples[p] = (x, w, first); triples[q] = (x, w, 1 - first)
            before = e.workers[w].free[0]
            got = _start_checked(a, e, triples)
            kinds = got["kind"].tolist()
            assert kinds[p] == K.HQ_START_PREFILLED and kinds[q] == K.HQ_START_REPEAT and got["accepted"] == 1
            assert a.assigned_lookup([x])[1].tolist() == [first] == [e.tasks[x].rv]
            assert before - e.workers[w].free[0] == core.amount(2 if first == 0 else 1)  # the free row is that variant's (the device's equals the mirror's)
        # (the audit has compared the (row, slot) counts with the entries after every batch)  Finished, every task gives back what its variant took
        gf._finish_checked(a, e, [(x, w) for x in pf])
        assert a.assigned_count() == 0 and e.workers[w].free[0] == core.amount(64)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 4: batch sizes at the edges, twin contexts
def _mixed_env(rng, n, ctxs):
    """three large workers; about n tasks: assigned (two request shapes, either variant), prefilled, Retracting in their queue, waiting -- on every context"""
    e = SchedEnv(abi.make_config(**CFG))
    ws = e.new_workers_cpus([1000, 1000, 1000])
    shapes = [TB().cpus(1), TB().cpus(2).next_variant().cpus(1)]
    retr = []
    for _ in range(max(n, 4)):
        k = int(rng.integers(0, len(shapes)))
        x = e.new_task(shapes[k]); w = ws[int(rng.integers(0, 3))]
        u = rng.random()
        if u < 0.5:
            e.assign_task(x, w, int(rng.integers(0, k + 1)))
        elif u < 0.8:
            _prefill_by_hand(e, x, w)
        elif u < 0.9:
            retr.append((x, w))
    for t in ctxs:
        cc.seed_ledger(t, e)
    for x, w in retr:
        e.tasks[x].state, e.tasks[x].worker = core.RETRACTING, w
    for t in ctxs:
        if retr:
            t.retracting_add([x for x, _ in retr], [w for _, w in retr])
        cc.seed_ready_graph(t, e)
    return e, ws


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_against_the_parents_sequence(n):
    """a random batch of n positions with refused ones among them; context A takes the one call, context B hqtick_assigned_start_prefilled +
    hqtick_retracting_started of the positions the mirror accepted; both equal SchedEnv.start_tasks"""
    rng = np.random.default_rng(7300 + n)
    a, b = _ctx(), _ctx()
    try:
        e, ws = _mixed_env(rng, n, (a, b))
        pool = sorted(e.tasks)
        triples = []
        for _ in range(n):
            x = pool[int(rng.integers(0, len(pool)))]
            t = e.tasks[x]
            u = rng.random()
            w = t.worker if t.worker is not None and u < 0.8 else ws[int(rng.integers(0, 3))]
            v = (t.rv if t.state == core.ASSIGNED else 0) if rng.random() < 0.8 else int(rng.integers(0, 3))
            triples.append((x, w, v) if u < 0.95 else (10**12 + int(rng.integers(0, 9)), w, 0))
        got = _start_checked(a, e, triples)
        kinds = got["kind"].tolist()
        if n >= 63:
            assert any(k not in ACC for k in kinds) and any(k in ACC for k in kinds)
        started = [(x, v) for (x, w, v), k in zip(triples, kinds) if k == K.HQ_START_PREFILLED]
        retr = [(x, w, e.tasks[x].rq, v, e.tasks[x].priority) for (x, w, v), k in zip(triples, kinds) if k == K.HQ_START_RETRACTING]
        assert b.assigned_start_prefilled(started) == len(started)
        assert b.retracting_started(retr) == len(retr)
        ids = sorted(e.tasks)
        va, vb = (dict(ready=t.ready_count(), sn=t.assigned_count(), pf=t.assigned_prefilled_count(), retr=t.retracting_count(), free=t.assigned_free_rows().tolist(),
                       worker=t.assigned_lookup(ids)[0].tolist(), variant=t.assigned_lookup(ids)[1].tolist()) for t in (a, b))
        assert va == vb
        _clean(b)
        # what the parent's two calls started reads 1 there too; an Assigned task that started is what the parent could not tell
        by_b = {s[0] for s in started} | {s[0] for s in retr}
        for x, r in zip(ids, b.assigned_running(ids).tolist()):
            assert r in ((1,) if x in by_b else (0, NO_ENTRY)), x
        _lose_worker(a, e, ws[0])  # started prefilled and Retracting tasks are among the lost worker's running tasks, merely assigned and prefilled ones are not
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 5: the claim words go back
def test_claim_words_are_restored():
    """a started entry stays in the table; were its claim word left at the position that started it, every later batch that names the id at a HIGHER position would
    lose its claim against that stale position: the finish and the cancel below would answer _REPEAT / no route"""
    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        ws = e.new_workers_cpus([400, 400])
        k = 70
        groups = [[e.new_task(TB().cpus(1)) for _ in range(k)] for _ in range(3)]
        for g in groups:
            for j, x in enumerate(g):
                e.assign_task(x, ws[j % 2])
        pf = [e.new_task(TB().cpus(1)) for _ in range(k)]
        for j, x in enumerate(pf):
            _prefill_by_hand(e, x, ws[j % 2])
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        first = [(x, e.tasks[x].worker, 0) for g in groups for x in g] + [(x, e.tasks[x].worker, 0) for x in pf]
        got = _start_checked(a, e, first)
        assert got["accepted"] == 4 * k and set(got["kind"].tolist()) == {K.HQ_START_ASSIGNED, K.HQ_START_PREFILLED}
        pad = [10**12 + j for j in range(300)]  # every id now sits at a higher position than the one that started it
        fin = [(x, ws[0]) for x in pad] + [(x, e.tasks[x].worker) for x in groups[0] + pf[: k // 2]]
        got = gf._finish_checked(a, e, fin)
        assert got["kind"].tolist() == [K.HQ_FINISH_NONE] * len(pad) + [K.HQ_FINISH_ASSIGNED] * (k + k // 2)
        ids = pad + groups[1] + pf[k // 2:]
        want = e.cancel_tasks(ids)
        got = a.cancel_tasks(ids)
        assert got["messages"] == {w: xs for w, xs in sorted(want.items())}
        assert got["route_kind"].tolist() == [K.HQ_CANCEL_NONE] * len(pad) + [K.HQ_CANCEL_ASSIGNED] * (k + k - k // 2)
        again = [(x, ws[0], 0) for x in pad] + [(x, e.tasks[x].worker, 0) for x in groups[2]]
        got = _start_checked(a, e, again)
        assert got["kind"].tolist() == [K.HQ_START_NONE] * len(pad) + [K.HQ_START_RUNNING] * k and got["accepted"] == 0
        assert a.assigned_count() == k and (a.assigned_free_rows() == cc.free_rows(e)).all()
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 6: the running byte and a table rebuild
def test_running_byte_survives_a_rebuild_and_a_repack():
    """100 entries in the first table of 1024 buckets, half of them started; 450 more entries make (100 + 450) x 2 > 1024: the table is rebuilt.  Then a worker
    joins and leaves (the rows are re-packed).  The bits are where they were; what entered by hqtick_assigned_add, a seed and hqtick_assigned_add_mn reads 0."""
    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        ws = e.new_workers_cpus([2000, 2000, 4, 4])
        old = [e.new_task(TB().cpus(1)) for _ in range(100)]
        for j, x in enumerate(old):
            e.assign_task(x, ws[j % 2])
        e.rq_id(TB().n_nodes(2))
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        ran = old[::2]
        _start_checked(a, e, [(x, e.tasks[x].worker, 0) for x in ran])
        new = [e.new_task(TB().cpus(1)) for _ in range(450)]
        for j, x in enumerate(new):
            e.assign_task(x, ws[j % 2])
        assert a.assigned_add([(x, e.tasks[x].worker, e.tasks[x].rq, 0, e.tasks[x].priority) for x in new]) == 450
        mn = e.new_task(TB().n_nodes(2)); e.start_task_mn(mn, [ws[2], ws[3]])
        assert a.assigned_add_mn([(mn, e.tasks[mn].rq, e.tasks[mn].priority, [ws[2], ws[3]])]) == 1
        seeded = e.new_task(TB().cpus(1)); _prefill_by_hand(e, seeded, ws[0])
        assert a.assigned_track_prefilled([(seeded, ws[0], e.tasks[seeded].rq, e.tasks[seeded].priority)]) == 1
        late = new + [mn, seeded]  # the graph knows them too; they are held, not queued
        assert len(a.graph_add_tasks(late, [e.tasks[x].priority for x in late], [e.tasks[x].rq for x in late], [[] for _ in late])) == len(late)
        assert a.ready_remove(late) == len(late)
        wn = e.new_worker(WB(3))
        a.cluster_add_workers([wn], [[core.amount(3)]])
        assert e.remove_worker(wn) == [] and a.cluster_remove_workers([wn]) == [] and a.cluster_last_requeued_running() == []
        ids = old + new + [mn, seeded]
        want = [1 if x in set(ran) else 0 for x in ids]
        assert a.assigned_running(ids).tolist() == want
        _clean(a)
        got = a.start_tasks(*_cols(e, [(x, e.tasks[x].worker, 0) for x in old]))  # the started half answers _RUNNING, the other half starts
        assert got["kind"].tolist() == [K.HQ_START_RUNNING if x in set(ran) else K.HQ_START_ASSIGNED for x in old] and got["accepted"] == 50
        assert a.assigned_running(ids).tolist() == [1] * 100 + [0] * 452
        _clean(a)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 7: the batch order under saturation
@pytest.mark.parametrize("order", ["prefilled_first", "retracting_first"])
def test_order_under_saturation(order):
    """w2 (2 cpus) holds the redirect's entry of a Retracting task (1 cpu) and a prefilled task that asks for 2.  _PREFILLED first: free 1 -> 0 (saturated), then the
    Retracting start gives the redirect's cpu back: 1.  _RETRACTING first: 2, then 0.  The device follows the batch order as the reference's loop does."""
    a = _ctx(reserve=1, fill_max=1)
    try:
        e = SchedEnv(abi.make_config(reserve=1, fill_max=1, **CFG))
        e.rq_id(TB()); big = e.rq_id(TB().cpus(2))  # (the ledger learns the 2-cpu request with the first tick's snapshot)
        tasks = e.new_tasks(3, TB())
        w1 = e.new_worker(WB(1))
        snap = e.snapshot()
        a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
        e.apply(_tick(a, snap))
        w2 = e.new_worker(WB(2))
        a.cluster_add_workers([w2], [[core.amount(2)]])
        e.apply(_tick(a, e.snapshot()))
        (t,) = [x for x in tasks if e.task(x).is_retracting()]
        assert e.task(t).worker == w1 and e.redirects[t][0] == w2 and a.retracting_count() == 1
        (on_w2,) = [x for x in e.workers[w2].assigned_tasks if x != t]
        e.finish_task(on_w2, w2)
        assert a.assigned_release([on_w2]) == 1
        pf = e.new_task(TB().cpus(2))
        assert e.tasks[pf].rq == big
        _prefill_by_hand(e, pf, w2)
        assert a.assigned_track_prefilled([(pf, w2, big, e.tasks[pf].priority)]) == 1
        cc.seed_ready_graph(a, e)
        assert e.workers[w2].free[0] == core.amount(1)
        batches = {"prefilled_first": [(pf, w2, 0), (t, w1, 0)], "retracting_first": [(t, w1, 0), (pf, w2, 0)]}
        ends = {}
        for name, batch in batches.items():
            m = copy.deepcopy(e)
            assert m.start_tasks(batch) == 2
            ends[name] = m.workers[w2].free[0]
        assert ends == {"prefilled_first": core.amount(1), "retracting_first": 0}  # the two orders differ: the test means something
        got = _start_checked(a, e, batches[order], overfull=True)
        assert sorted(got["kind"].tolist()) == sorted([K.HQ_START_PREFILLED, K.HQ_START_RETRACTING])
        assert e.workers[w2].free[0] == ends[order]
        row = sorted(e.workers).index(w2)
        assert int(a.assigned_free_rows()[row, 0]) == ends[order]
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 8: the call's rules
def _state(t, ids):
    s = t.graph_stats(); s.pop("last_kernel_us", None)
    return dict(ready=t.ready_count(), stats=s, sn=t.assigned_count(), pf=t.assigned_prefilled_count(), retr=t.retracting_count(), free=t.assigned_free_rows().tolist(),
                run=t.assigned_running(ids).tolist(), kinds=t.start_last_routes().tolist())


def test_call_rules():
    from hyperqueue_amd.tick import HqTickError

    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        ws = e.new_workers_cpus([4, 4])
        held = [e.new_task(TB().cpus(1)) for _ in range(2)]
        e.assign_task(held[0], ws[0]); e.assign_task(held[1], ws[1])
        queued = [e.new_task(TB().cpus(1)) for _ in range(5)]
        with pytest.raises(HqTickError) as err:  # no resident ready set
            a.start_tasks(held, ws, [0, 0])
        assert err.value.code == abi.HQTICK_E_INVALID
        a.cluster_upload(e.snapshot())
        cc.seed_ready_graph(a, e)
        with pytest.raises(HqTickError) as err:  # ledger off
            a.start_tasks(held, ws, [0, 0])
        assert err.value.code == abi.HQTICK_E_INVALID and "assignment ledger not enabled" in str(err.value)
        cc.seed_ledger(a, e)
        _start_checked(a, e, [(held[0], ws[0], 0)])
        before = _state(a, held)
        assert before["kinds"] == [K.HQ_START_ASSIGNED] and before["run"] == [1, 0]
        f = a._lib.hqtick_start_tasks
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u8p, abi.u32p, abi.u64p]
        ids = np.asarray(held, np.uint64); wid = np.asarray(ws, np.uint32); var = np.zeros(2, np.uint8); rq = np.zeros(2, np.uint32); pr = np.zeros(2, np.uint64)
        p = lambda x, ty: x.ctypes.data_as(ty)
        for args in ((None, p(wid, abi.u32p), p(var, abi.u8p)), (p(ids, abi.u64p), None, p(var, abi.u8p)), (p(ids, abi.u64p), p(wid, abi.u32p), None)):  # a null array
            assert f(a._ctx, 2, *args, p(rq, abi.u32p), p(pr, abi.u64p)) == abi.HQTICK_E_INVALID
        assert f(a._ctx, (1 << 26) + 1, p(ids, abi.u64p), p(wid, abi.u32p), p(var, abi.u8p), None, None) == abi.HQTICK_E_CAPACITY  # (refused before anything is read)
        assert _state(a, held) == before
        # rq / priority may be NULL while the Retracting table is empty, and not once it holds a task
        a.retracting_add([queued[0]], [ws[0]]); e.tasks[queued[0]].state, e.tasks[queued[0]].worker = core.RETRACTING, ws[0]
        before = _state(a, held)
        for args in ((None, p(pr, abi.u64p)), (p(rq, abi.u32p), None), (None, None)):
            assert f(a._ctx, 2, p(ids, abi.u64p), p(wid, abi.u32p), p(var, abi.u8p), *args) == abi.HQTICK_E_INVALID
        assert _state(a, held) == before
        got = a.start_tasks([], [], [])  # n = 0: an empty kind list
        assert got["accepted"] == 0 and len(got["kind"]) == 0 and a.assigned_last_unknown() == 0
        _start_checked(a, e, [(queued[0], ws[0], 0)])  # ... and the Retracting task in its queue starts on the worker it was retracting from
        assert a.retracting_count() == 0 and a.assigned_running([queued[0]]).tolist() == [1]
        got = a.start_tasks([held[1]], [ws[1]], [0])  # the table is empty again: NULL rq / priority
        assert got["kind"].tolist() == [K.HQ_START_ASSIGNED]
        e.start_tasks([(held[1], ws[1], 0)])
        # a two-call tick's placement is pending: refused, nothing changes, and the consume still finds its selection
        res = _tick(a, e.snapshot(), resident=True)
        assert sum(len(r) for r in res.records) == 4
        with pytest.raises(HqTickError) as err:
            a.start_tasks(held, ws, [0, 0])
        assert err.value.code == abi.HQTICK_E_INVALID and "pending" in str(err.value)
        a.ready_consume_last(); e.apply(res)
        assert a.assigned_running(held).tolist() == [1, 1]
        placed = [x for x in queued[1:] if e.tasks[x].state == core.ASSIGNED]
        got = _start_checked(a, e, [(x, e.tasks[x].worker, e.tasks[x].rv) for x in placed])
        assert got["accepted"] == len(placed) == 4
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 9: the audit mode
def test_audit_mode_runs_the_scenario():
    """a context created with HQTICK_CHECK_RESIDENT=1 audits itself after every call that changes resident state: scenario 1 runs through (a child process: the
    variable is read when the library creates the context)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_start as g\n"
            "a = g._ctx()\ng._run_running_task(a)\na.close()\nprint('AUDITED-OK')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HQTICK_CHECK_RESIDENT="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "AUDITED-OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- 10: one larger batch
def test_one_larger_batch_then_finished_against_the_twin():
    """one tick of the 100 000-task x 256-worker workload consumed; every assigned task started in one call, shuffled, then finished; the twin finishes alone"""
    snap = workloads.make_steady("c3p", seed=3, n_tasks=100_000, n_workers=256)
    W, R = len(snap.worker_id), snap.n_resources
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    ids, prio, rqs = np.asarray(snap.task_id, np.uint64), np.asarray(snap.task_priority, np.uint64), np.asarray(snap.task_rq, np.uint32)
    kw = dict(flags=abi.HQTICK_FLAG_CONSUME_IN_TICK | abi.HQTICK_FLAG_NO_KERNEL_TIMING)
    a, b = _ctx(**kw), _ctx(**kw)
    try:
        scn = snap.to_c(resident_workers=True)
        scn.assigned_off = None; scn.assigned_rq = None; scn.assigned_variant = None; scn.prefilled_off = None; scn.prefilled_rq = None
        no_deps = (np.zeros(len(ids) + 1, np.uint32), np.zeros(0, np.uint64))
        results = []
        for t in (a, b):
            t.cluster_upload(snap)
            t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
            assert len(t.graph_add_tasks(ids, prio, rqs, no_deps)) == len(ids)
            t.assigned_enable([]); t.assigned_track_prefilled([])
            results.append(abi.parse_result(t.tick_raw(scn, resident=True), W, R))
        res = results[0]
        assert res.records == results[1].records
        wid = snap.worker_id.tolist()
        asg = [(tid, wid[w], v) for w, recs in enumerate(res.records) for (tid, v, k) in recs if k == abi.HQ_REC_ASSIGN]
        n_pf = a.assigned_prefilled_count()
        assert len(asg) > 1000 and a.assigned_count() == len(asg)
        order = np.random.default_rng(12).permutation(len(asg))
        s_ids = np.asarray([asg[k][0] for k in order], np.uint64); s_ws = np.asarray([asg[k][1] for k in order], np.uint32); s_v = np.asarray([asg[k][2] for k in order], np.uint8)
        free = a.assigned_free_rows().copy()
        assert not a.assigned_running(s_ids).any()
        got = a.start_tasks(s_ids, s_ws, s_v)
        assert got["accepted"] == len(asg) and (got["kind"] == K.HQ_START_ASSIGNED).all() and a.assigned_last_unknown() == 0
        assert (a.assigned_running(s_ids) == 1).all() and (a.assigned_free_rows() == free).all() and a.assigned_count() == len(asg) and a.assigned_prefilled_count() == n_pf
        got = a.start_tasks(s_ids, s_ws, s_v)
        assert got["accepted"] == 0 and (got["kind"] == K.HQ_START_RUNNING).all()
        fa = a.finish_tasks(s_ids, s_ws); fb = b.finish_tasks(s_ids, s_ws)
        assert fa["accepted"] == fb["accepted"] == len(asg) and (fa["kind"] == K.HQ_FINISH_ASSIGNED).all()
        assert (a.assigned_free_rows() == b.assigned_free_rows()).all() and a.assigned_count() == b.assigned_count() == 0
        assert a.assigned_prefilled_count() == b.assigned_prefilled_count() == n_pf and a.ready_count() == b.ready_count()
        r = a.resident_check(abi.HQ_CHECK_ALL)
        assert r["n_failed"] == 0, r["failed"]
    finally:
        a.close(); b.close()
