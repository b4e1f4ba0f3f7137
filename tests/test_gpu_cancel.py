"""hqtick_cancel_tasks (include/hqtick.h) on the device: the reference's four cancel scenarios through graph + ready set + ledger with prefilled
tracking, twin contexts (the one call against today's hqtick_graph_remove + hqtick_assigned_release + hqtick_assigned_unprefill) on random histories checked
against SchedEnv.cancel_tasks, Retracting tasks with a redirect, a context without a graph, the call's rules, and one larger batch."""
import numpy as np
import pytest

import cancel_cases as cc
from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

pytestmark = pytest.mark.gpu

AUDIT = abi.HQ_CHECK_ALL | abi.HQ_CHECK_STRICT
CFG = dict(time_limit_s=20.0)


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


def _cancel_checked(a, e, ids):
    """the batch on the mirror and on context a: messages, routes, closure, ready set and free rows must agree"""
    before = {x for x, tk in e.tasks.items() if tk.state != core.FINISHED}
    want = e.cancel_tasks(ids)
    routes = e.last_cancel_routes
    closure = sorted(before - {x for x, tk in e.tasks.items() if tk.state != core.FINISHED})
    got = a.cancel_tasks(ids)
    assert got["messages"] == want
    assert got["n_ids"] == sum(len(v) for v in want.values())
    assert got["route_worker"].tolist() == [abi.HQ_NO_WORKER if w is None else w for (w, _) in routes]
    assert got["route_kind"].tolist() == [k for (_, k) in routes]
    assert a.ready_count() == sum(len(s) for s in e.ready.values())
    assert (a.assigned_free_rows() == cc.free_rows(e)).all()
    return got, closure


# ---------------------------------------------------------------------------------------------- the reference's scenarios
@pytest.mark.parametrize("name", ["task_cancel", "mn_cancel", "prefill_cancel"])
def test_reference_scenarios(name):
    from hyperqueue_amd.tick import Tick

    b = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))  # the mirror's scheduler
    a = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))
    try:
        e, ids, want, survivors = {"task_cancel": cc.scenario_task_cancel, "mn_cancel": cc.scenario_mn_cancel, "prefill_cancel": lambda: cc.scenario_prefill_cancel(b)}[name]()
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        _clean(a)
        got, closure = _cancel_checked(a, e, ids)
        assert got["messages"] == want
        assert got["closure"].tolist() == closure and got["graph_unknown"] == 0
        assert sorted(x for x, tk in e.tasks.items() if tk.state != core.FINISHED) == sorted(survivors)
        assert a.assigned_mn_count() == 0 and a.assigned_prefilled_count() == 0
        assert a.assigned_count() == sum(len(w.assigned_tasks) for w in e.workers.values())
        if name == "mn_cancel":
            assert all(f & abi.HQ_WORKER_SN for f in a.cluster_worker_flags().tolist())
        _clean(a)
    finally:
        a.close(); b.close()


def _retracting_pair(a):
    """test_reactor.rs:993-1007 with context a as the scheduler AND the ledger host: -> (mirror, w1, w2, the Retracting task, the other two)"""
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


def test_steal_cancel_and_the_redirect():
    """a Retracting task with a redirect: the message goes to the worker it is retracting FROM, the target's free row comes back, the table's count drops and a
    late retract response reassigns nothing"""
    from hyperqueue_amd.tick import Tick

    a = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))
    try:
        e, w1, w2, t, others = _retracting_pair(a)
        cc.seed_ready_graph(a, e)
        _clean(a)
        lw, _ = a.assigned_lookup([t])
        assert lw.tolist() == [w2]  # the ledger names the redirect TARGET
        free_before = a.assigned_free_rows().copy()
        got, closure = _cancel_checked(a, e, [t, t])
        assert got["messages"] == {w1: [t]} and closure == [t] and got["closure"].tolist() == [t]
        assert got["route_kind"].tolist() == [abi.HQ_CANCEL_RETRACTING, abi.HQ_CANCEL_REPEAT]
        assert a.retracting_count() == 0
        i2 = sorted(e.workers).index(w2)
        assert a.assigned_free_rows()[i2, 0] == free_before[i2, 0] + core.amount(1)
        assert a.assigned_lookup([t])[0].tolist() == [abi.HQ_NO_WORKER]
        assert a.retract_response(w1, [t]) == []
        _clean(a)
    finally:
        a.close()


def test_retracting_without_a_redirect_gets_its_route_from_the_table_alone():
    from hyperqueue_amd.tick import Tick

    b = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))
    a = Tick(abi.make_config(reserve=1, fill_max=1, **CFG))
    try:
        e, w1, tasks, assigned, prefilled = cc.setup_prefill(b)
        cc.seed_ledger(a, e)
        e.new_task(TB().cpus(1).user_priority(10))  # dissolves the prefill set: Retracting{w1} in its queue (process_retracted)
        assert e.retract_messages == [(w1, prefilled)]
        assert a.assigned_unprefill([prefilled]) == 1
        a.retracting_add([prefilled], [w1])
        cc.seed_ready_graph(a, e)
        _clean(a)
        n_ready = a.ready_count()
        got, closure = _cancel_checked(a, e, [prefilled])
        assert got["messages"] == {w1: [prefilled]} and got["route_kind"].tolist() == [abi.HQ_CANCEL_RETRACTING]
        assert got["ready_removed"] == 1 and a.ready_count() == n_ready - 1 and a.retracting_count() == 0
        _clean(a)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- twin contexts
def _fits(e, w, rq, v):
    for (r, kind, amt) in e.requests[rq][v]["entries"]:
        free = w.free[r] if r < len(w.free) else 0
        tot = w.total[r] if r < len(w.total) else 0
        if (kind == abi.HQ_ENTRY_AMOUNT and amt > free) or (kind != abi.HQ_ENTRY_AMOUNT and (free != tot or tot == 0)):
            return False
    return True


def _prefill_by_hand(e, tid, wid):
    t = e.tasks[tid]
    t.state, t.worker = core.PREFILLED, wid
    e.workers[wid].prefilled_tasks.add(tid)
    e.ready[t.rq].discard(tid)
    if t.rq not in e.prefill or len(e.prefill[t.rq][1]) == 0:
        e.prefill[t.rq] = (t.priority, core.task_id_set())
    e.prefill[t.rq][1].insert(tid)


def _random_env(rng, W):
    """W workers of two resources, the first a 512-cpu one holding 400 one-cpu tasks; the others filled with tasks of ALL, fractional and two-variant requests,
    one two-node task, prefilled tasks, a queue of ready tasks and chains of consumers behind tasks in every state"""
    e = SchedEnv(abi.make_config(reserve=0, fill_max=2, **CFG))
    gpu = e.new_named_resource("gpus")
    shapes = [TB().cpus(1), TB().cpus(2), TB().cpus_all(), TB().cpus(0.5), TB().cpus(3).next_variant().cpus(1), TB().cpus(1).add_resource(gpu, 1),
              TB().cpus(1).add_all(gpu), TB().add_resource(gpu, 0.5)]
    big = e.new_worker(WB(512).res_sum("gpus", 2))
    rest = [e.new_worker(WB(int(rng.integers(3, 8))).res_sum("gpus", 2)) for _ in range(W - 1)]
    for _ in range(400):
        x = e.new_task(TB().cpus(1))
        e.assign_task(x, big)
        if rng.random() < 0.5:
            e.start_task(x)
    mn = e.new_task(TB().n_nodes(2))
    e.start_task_mn(mn, [rest[-1], rest[0]])
    for wid in rest[1:-1]:
        w = e.workers[wid]
        for _ in range(int(rng.integers(0, 5))):
            b = shapes[int(rng.integers(0, len(shapes)))]
            rq = e.rq_id(b)
            v = int(rng.integers(0, len(e.requests[rq])))
            if _fits(e, w, rq, v):
                x = e.new_task(b)
                e.assign_task(x, wid, v)
                if rng.random() < 0.5:
                    e.start_task(x, v)
        if rng.random() < 0.5:
            _prefill_by_hand(e, e.new_task(TB().cpus(1)), wid)
    for _ in range(700):
        e.new_task(shapes[int(rng.integers(0, len(shapes)))])
    live = [x for x, tk in e.tasks.items()]
    for _ in range(60):  # consumers, and consumers of consumers
        p = live[int(rng.integers(0, len(live)))]
        c = e.new_task(TB().cpus(1).task_deps([p]))
        if rng.random() < 0.5:
            e.new_task(TB().cpus(1).task_deps([c, live[int(rng.integers(0, len(live)))]]))
    return e, big


def _view(t, ids):
    w, v = t.assigned_lookup(ids)
    return dict(ready=t.ready_count(), sn=t.assigned_count(), mn=t.assigned_mn_count(), pf=t.assigned_prefilled_count(), free=t.assigned_free_rows().tolist(),
                worker=w.tolist(), variant=v.tolist(), flags=t.cluster_worker_flags().tolist())


def _batch(rng, e, size, must=()):
    pool = [x for x, tk in sorted(e.tasks.items()) if tk.state not in (core.FINISHED, core.RETRACTING) and x not in must]
    rng.shuffle(pool)
    n_rep = size // 8 if size > 3 else 0
    n_unknown = size // 16 if size > 3 else 0
    take = list(must) + pool[:max(0, size - n_rep - n_unknown - len(must))]
    ids = take + [take[int(rng.integers(0, len(take)))] for _ in range(n_rep)] + [10**12 + int(rng.integers(0, 1000)) for _ in range(n_unknown)]
    ids += [10**12 + 5000 + k for k in range(size - len(ids))]
    rng.shuffle(ids)
    return [int(x) for x in ids[:size]]


@pytest.mark.parametrize("W", [3, 70, 300])
def test_twin_contexts_on_a_random_history(W):
    """context A cancels with the one call, context B with today's three; after every batch both show the same ready set, ledger, worker flags and next tick, and
    A's messages and routes are the mirror's"""
    from hyperqueue_amd.tick import HqTickError, Tick

    rng = np.random.default_rng(7700 + W)
    e, big = _random_env(rng, W)
    a, b = Tick(e.config), Tick(e.config)
    try:
        for t in (a, b):
            cc.seed_ledger(t, e); cc.seed_ready_graph(t, e)
        _clean(a)
        ever = sorted(e.tasks)
        assert _view(a, ever) == _view(b, ever)
        ticks = 0
        for size in (700, 1, 63, 64, 65, 257):
            must = sorted(e.workers[big].assigned_tasks)[:300] if size == 700 else ()
            ids = _batch(rng, e, size, must)
            got, closure = _cancel_checked(a, e, ids)
            if size == 700:
                assert len(got["messages"][big]) > 256
            assert b.graph_remove(ids, recursive=True).tolist() == closure == got["closure"].tolist()
            b.assigned_release(ids); b.assigned_unprefill(ids)
            ever = sorted(e.tasks)
            assert _view(a, ever) == _view(b, ever)
            _clean(a)
            # the next tick, on the resident ready set, two-call form
            snap = e.snapshot()
            try:
                ra = _tick(a, snap, resident=True)
            except HqTickError as err:
                assert err.code == abi.HQTICK_E_UNSUPPORTED
                with pytest.raises(HqTickError):
                    _tick(b, snap, resident=True)
                continue
            rb = _tick(b, snap, resident=True)
            assert ra.records == rb.records and ra.retracts == rb.retracts and ra.redirects == rb.redirects and ra.mn == rb.mn and (ra.new_free == rb.new_free).all()
            a.ready_consume_last(); b.ready_consume_last()
            e.apply(ra)
            ticks += 1
            assert _view(a, ever) == _view(b, ever)
        assert ticks >= 1  # (a tick the library refuses as unsupported is refused on both contexts alike; not every one of the history may be)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- without a graph, the call's rules, one larger batch
def test_without_a_graph():
    from hyperqueue_amd.tick import Tick

    a = Tick(abi.make_config(**CFG))
    try:
        e, ids, want, survivors = cc.scenario_task_cancel()
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e, graph=False)
        ready = sorted(x for s in e.ready.values() for x in s)
        listed_ready = [x for x in ids if x in ready]
        got = a.cancel_tasks(ids)
        assert got["messages"] == want and len(got["closure"]) == 0
        assert got["ready_removed"] == len(listed_ready) and a.ready_count() == len(ready) - len(listed_ready)  # the listed ids alone: no graph, no closure
        assert a.assigned_count() == 0 and (a.assigned_free_rows() == a.assigned_free_rows()[:, :1] * 0 + core.amount(10)).all()
        assert _clean(a)["checked"] & abi.HQ_CHECK_LEDGER
    finally:
        a.close()


def test_call_rules():
    from hyperqueue_amd.tick import HqTickError, Tick

    a = Tick(abi.make_config(**CFG))
    try:
        e = SchedEnv(abi.make_config(**CFG))
        ws = e.new_workers_cpus([4, 4])
        held = [e.new_task(TB().cpus(1)) for _ in range(2)]
        e.assign_task(held[0], ws[0]); e.assign_task(held[1], ws[1])
        queued = [e.new_task(TB().cpus(1)) for _ in range(5)]
        with pytest.raises(HqTickError) as err:  # no resident ready set
            a.cancel_tasks(held)
        assert err.value.code == abi.HQTICK_E_INVALID
        a.cluster_upload(e.snapshot())
        cc.seed_ready_graph(a, e)
        with pytest.raises(HqTickError) as err:  # ledger off
            a.cancel_tasks(held)
        assert err.value.code == abi.HQTICK_E_INVALID and "assignment ledger not enabled" in str(err.value)
        assert a.ready_count() == 5
        cc.seed_ledger(a, e)
        got = a.cancel_tasks([])  # n = 0
        assert got["messages"] == {} and got["n_ids"] == 0 and len(got["route_kind"]) == 0 and got["ready_removed"] == 0
        # a two-call tick's placement is pending: refused, nothing changes, and the consume still finds its selection
        res = _tick(a, e.snapshot(), resident=True)
        n_placed = sum(len(r) for r in res.records)
        assert n_placed == 5
        with pytest.raises(HqTickError) as err:
            a.cancel_tasks(held + queued[:2])
        assert err.value.code == abi.HQTICK_E_INVALID and "pending" in str(err.value)
        assert a.ready_count() == 5 and a.assigned_count() == 2 and a.assigned_lookup(held)[0].tolist() == ws
        a.ready_consume_last()
        e.apply(res)
        assert a.ready_count() == 0 and a.assigned_count() == 7
        got, closure = _cancel_checked(a, e, held + queued[:2])
        assert got["n_ids"] == 4 and a.assigned_count() == 3
        _clean(a)
    finally:
        a.close()


def test_one_larger_batch_against_the_twin():
    """1024 workers, 20 000 ledger entries (2 000 of them prefilled), a batch of 20 000 ids: the one call against hqtick_ready_remove + hqtick_assigned_release +
    hqtick_assigned_unprefill, the messages against hqtick_assigned_lookup grouped on the host (what a host does today)"""
    from hyperqueue_amd.tick import Tick

    rng = np.random.default_rng(99)
    W = 1024
    e = SchedEnv(abi.make_config(**CFG))
    ws = e.new_workers_cpus([64] * W)
    rqs = [e.rq_id(TB().cpus(1)), e.rq_id(TB().cpus(2))]
    n_sn, n_pf, n_ready = 18_000, 2_000, 5_000
    ids = (np.arange(n_sn + n_pf + n_ready, dtype=np.uint64) * 3 + 1000)
    rng.shuffle(ids)
    sn, pf, ready = ids[:n_sn], ids[n_sn:n_sn + n_pf], np.sort(ids[n_sn + n_pf:])
    sn_w = rng.integers(0, W, n_sn); sn_q = rng.integers(0, 2, n_sn)
    used = np.bincount(sn_w, weights=(sn_q + 1), minlength=W).astype(np.int64)
    assert used.max() <= 64
    for i, wid in enumerate(ws):
        e.workers[wid].free[0] -= int(used[i]) * core.amount(1)
    snap = e.snapshot()
    entries = [(int(t), ws[int(w)], rqs[int(q)], 0, 0) for t, w, q in zip(sn, sn_w, sn_q)]
    pf_entries = [(int(t), ws[int(w)], rqs[0], 0) for t, w in zip(pf, rng.integers(0, W, n_pf))]
    a, b = Tick(e.config), Tick(e.config)
    try:
        for t in (a, b):
            t.cluster_upload(snap); t.assigned_enable(entries)
            assert t.assigned_track_prefilled(pf_entries) == n_pf
            t.upload_ready(ready, np.zeros(n_ready, np.uint64), np.full(n_ready, rqs[0], np.uint32))
        batch = np.concatenate([sn[:15_000], pf[:1_500], ready[:2_000], sn[:500], np.arange(1_000, dtype=np.uint64) + 10**12])
        rng.shuffle(batch)
        assert len(batch) == 20_000
        lw, lv = b.assigned_lookup(batch)  # today's way to the messages: look the ids up, group on the host, first mention of an id only
        first = np.zeros(len(batch), bool); first[np.unique(batch, return_index=True)[1]] = True
        want = {}
        for t, w, f in zip(batch.tolist(), lw.tolist(), first.tolist()):
            if f and w != abi.HQ_NO_WORKER:
                want.setdefault(w, []).append(t)
        got = a.cancel_tasks(batch)
        assert got["messages"] == want and got["n_ids"] == 16_500 and got["ready_removed"] == 2_000
        kinds = np.bincount(got["route_kind"], minlength=6).tolist()
        assert kinds == [3_000, 15_000, 1_500, 0, 0, 500]
        assert b.ready_remove(batch) == 2_000
        assert b.assigned_release(batch) == 15_000 and b.assigned_unprefill(batch) == 1_500
        assert _view(a, ids) == _view(b, ids)
        assert a.assigned_count() == 3_000 and a.assigned_prefilled_count() == 500 and a.ready_count() == 3_000
        r = a.resident_check(abi.HQ_CHECK_ALL)
        assert r["n_failed"] == 0, r["failed"]
    finally:
        a.close(); b.close()
