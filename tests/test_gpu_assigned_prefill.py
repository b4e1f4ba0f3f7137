"""Prefilled tasks in the assignment ledger (hqtick_assigned_track_prefilled / _start_prefilled / _unprefill / _prefilled_count,
hqtick_cluster_last_requeued_prefilled).  As in test_gpu_assigned_mn.py, context A keeps the ledger — here with prefilled tracking on and NO
prefilled CSR in its snapshots — and context B runs today's protocol on SchedEnv's full snapshot (its worker_map_rank included): every tick of A equals B's, and
after every event A's free rows, assigned tasks and prefilled tasks equal SchedEnv's."""
import dataclasses
import os

import numpy as np
import pytest

from hyperqueue_amd import abi

pytestmark = pytest.mark.gpu

WAITING, ASSIGNED, RUNNING, PREFILLED, RETRACTING = 0, 1, 2, 3, 4
PF = 0xFE
COMPACT = abi.HQTICK_FLAG_COMPACT_RECORDS
DELTA16 = abi.HQTICK_FLAG_COMPACT_RECORDS | abi.HQTICK_FLAG_COMPACT_DELTA16
IN_TICK = abi.HQTICK_FLAG_CONSUME_IN_TICK
FORM_FLAGS = {"plain": 0, "compact": COMPACT, "delta16": DELTA16, "sink": 0}


def _same(a, b):
    assert a.status == b.status and a.is_optimal == b.is_optimal and a.batches == b.batches
    assert a.counts == b.counts and a.records == b.records and a.retracts == b.retracts
    assert (a.new_free == b.new_free).all()
    assert a.redirects == b.redirects and a.redirect_kinds == b.redirect_kinds
    assert a.mn == b.mn


def _strip(sc, prefilled=True):
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    if prefilled:
        sc.prefilled_off = None; sc.prefilled_rq = None
    return sc


def _ledger_tick(t, snap, prefilled_csr=False):
    """a tick of the ledger context: resident workers, resident Retracting table, no assigned CSR and (tracking on) no prefilled CSR"""
    sc = _strip(snap.to_c(resident_workers=True), prefilled=not prefilled_csr)
    sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None
    sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
    return abi.parse_result(t.tick_raw(sc), len(snap.worker_id), snap.n_resources)


def _b_snap(snap):
    # (with SchedEnv's own worker_map_rank: the resident worker set keeps the worker map with its removals, as core.worker_map does, so after a lost worker A
    # walks the workers in the reference's order and no longer in that of the remaining ids inserted afresh, which worker_map_rank=None stands for)
    return dataclasses.replace(snap, _keep=[])


def _n_kind(res, kind):
    return sum(1 for w in res.records for r in w if r[2] == kind)


def _view(t, ids):
    """everything the ledger shows of the listed ids and of the rows"""
    w, v = t.assigned_lookup(ids)
    return t.assigned_count(), t.assigned_prefilled_count(), w.tolist(), v.tolist(), t.assigned_free_rows().tolist()


def _check_state(e, t):
    snap = e.snapshot()
    W = len(snap.worker_id)
    assert t.cluster_workers().tolist() == sorted(e.workers)
    assert (t.assigned_free_rows() == np.asarray(snap.worker_free, np.uint64).reshape(W, snap.n_resources)).all()
    ids = sorted(e.tasks)
    w, v = t.assigned_lookup(ids)
    got_a, got_p = {}, {}
    for tid, wid, var in zip(ids, w.tolist(), v.tolist()):
        if wid == abi.HQ_NO_WORKER:
            assert var == 0xFF
        elif var == PF:
            got_p.setdefault(wid, set()).add(tid)
        else:
            got_a.setdefault(wid, set()).add((tid, var))
    want_a = {wid: {(x, e._assigned_variant(x, wid)) for x in w_.assigned_tasks} for wid, w_ in e.workers.items() if w_.assigned_tasks}
    want_p = {wid: set(w_.prefilled_tasks) for wid, w_ in e.workers.items() if w_.prefilled_tasks}
    assert got_a == want_a
    assert got_p == want_p
    assert t.assigned_count() == sum(len(x) for x in want_a.values())
    assert t.assigned_prefilled_count() == sum(len(x) for x in want_p.values())


# ---------------------------------------------------------------------------------------------- 1: fails without the feature
def _two_tick_env():
    """4 workers of 4 cpus, 24 one-cpu tasks, reserve 0, at most 2 prefilled tasks per worker: tick 1 assigns 16 and prefills 8"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB

    cfg = abi.make_config(reserve=0, fill_max=2, time_limit_s=20.0)
    e = SchedEnv(cfg)
    e.new_workers_cpus([4] * 4)
    for _ in range(24):
        e.new_task(TB().cpus(1))
    return cfg, e


def _between_the_ticks(e):
    """one assigned task of every worker finishes and 16 more tasks of the same request arrive.  (Without the finishes tick 2 could place nothing: a worker is
    prefilled only in a tick that also assigns it a task of the request, mapping.rs:185-196, and the arrivals go ahead of the prefilled block in their queue's
    take order, taskqueue.rs:320-355 — so every worker gets one ASSIGN record while it still holds its two prefilled tasks.)  -> (finished, new ids)"""
    from hyperqueue_amd.core import TaskBuilder as TB

    done = [min(w.assigned_tasks) for _, w in sorted(e.workers.items())]
    for x in done:
        e.finish_task(x, e.tasks[x].worker)
    return done, [e.new_task(TB().cpus(1)) for _ in range(16)]


def test_the_next_tick_does_not_prefill_workers_that_still_hold_prefilled_tasks():
    from hyperqueue_amd.tick import Tick

    cfg, e = _two_tick_env()
    a, b = Tick(cfg), Tick(cfg)
    try:
        snap = e.snapshot()
        a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
        want = b.tick(_b_snap(snap))
        _same(_ledger_tick(a, snap), want)
        assert _n_kind(want, abi.HQ_REC_PREFILL) >= 1
        e.apply(want)
        _check_state(e, a)
        done, _ = _between_the_ticks(e)
        assert a.assigned_release(done) == len(done)
        _check_state(e, a)
        snap = e.snapshot()
        want = b.tick(_b_snap(snap))
        assert _n_kind(want, abi.HQ_REC_ASSIGN) == 4
        blind = b.tick(dataclasses.replace(_b_snap(snap), prefilled=[[] for _ in snap.worker_id]))  # what a host that sent no prefilled CSR would get
        assert _n_kind(want, abi.HQ_REC_PREFILL) < _n_kind(blind, abi.HQ_REC_PREFILL)
        _same(_ledger_tick(a, snap), want)
        e.apply(want)
        _check_state(e, a)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 2: scenarios
N_SEEDS = 20
_STATS = {}  # seed -> counters of the scenario


class _Host:
    """the ledger host: what a reactor with the ledger and prefilled tracking on sends for each event, checked against SchedEnv"""

    def __init__(self, cfg):
        from hyperqueue_amd.tick import Tick

        self.a, self.b = Tick(cfg), Tick(cfg)
        self.uploaded = False

    def close(self):
        self.a.close(); self.b.close()

    def b_tick(self, snap):
        return self.b.tick(_b_snap(snap))

    def upload(self, snap):
        if not self.uploaded:
            self.a.cluster_upload(snap); self.a.assigned_enable([]); self.a.assigned_track_prefilled([])
            self.uploaded = True

    def tick(self, snap, want):
        _same(_ledger_tick(self.a, snap), want)

    def disposed(self, msgs, ready=None):
        """process_retracted outside a tick (reactor.rs:34-62): the tasks of a dissolved prefill set are Retracting in their queue.  ready: {task: (priority,
        rq)} when the context holds a resident ready set the host keeps current"""
        if not msgs or not self.uploaded:
            return
        msgs = sorted(msgs, key=lambda m: m[1])
        ids = [t for (_, t) in msgs]
        assert self.a.assigned_unprefill(ids) == len(ids) and self.a.assigned_last_unknown() == 0
        self.a.retracting_add(ids, [w for (w, _) in msgs])
        if ready is not None:
            self.a.ready_add(np.asarray(ids, np.uint64), np.asarray([ready[t][0] for t in ids], np.uint64), np.asarray([ready[t][1] for t in ids], np.uint32))

    def started(self, pairs):
        assert self.a.assigned_start_prefilled(pairs) == len(pairs) and self.a.assigned_last_unknown() == 0

    def released(self, batch):
        assert self.a.assigned_release(batch[:]) == len(batch) and self.a.assigned_last_unknown() == 0

    def unprefilled(self, ids):
        assert self.a.assigned_unprefill(ids) == len(ids) and self.a.assigned_last_unknown() == 0

    def blocked(self, wid, pairs):
        self.a.cluster_set_blocked(wid, pairs)

    def response(self, wid, tids, expect):
        assert self.a.retract_response(wid, tids) == expect

    def joined(self, wid, tot):
        self.a.cluster_add_workers([wid], tot, tot)

    def before_loss(self, snap):
        self.a.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)  # so that the requeued tasks have a resident ready set to go back into

    def lost(self, wid, sent, back, pf_back):
        assert self.a.cluster_remove_workers([wid]) == sent
        assert self.a.cluster_last_requeued() == back
        assert self.a.cluster_last_requeued_prefilled() == pf_back

    def ready_is(self, n):
        assert self.a.ready_count() == n

    def check(self, e):
        if self.uploaded:
            _check_state(e, self.a)
            assert self.a.retracting_count() == sum(1 for t in e.tasks.values() if t.state == RETRACTING)


class _OracleHost:
    """the generator alone, on the CPU: B is the oracle, there is no ledger context"""

    def __init__(self, cfg):
        from oracle.oracle import Oracle

        self.o = Oracle(cfg, canonical=True)

    def b_tick(self, snap):
        return self.o.tick(_b_snap(snap))

    def __getattr__(self, name):
        return lambda *a, **k: None


def _scenario(seed, host_cls=_Host):
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import HqTickError

    rng = np.random.default_rng(61_000 + seed)
    cfg = abi.make_config(reserve=int(rng.integers(0, 2)), fill_max=int((1, 3)[int(rng.integers(0, 2))]), time_limit_s=20.0)
    e = SchedEnv(cfg)
    h = host_cls(cfg)
    gpu = e.new_named_resource("gpus")
    shapes = [TB().cpus(1), TB().cpus(1), TB().cpus(1), TB().cpus(2), TB().cpus_all(), TB().cpus(0.5), TB().cpus(3).next_variant().cpus(1),
              TB().cpus(1).add_resource(gpu, 1), TB().cpus(1).add_all(gpu), TB().add_resource(gpu, 0.5)]
    for c in [int(x) for x in rng.integers(2, 6, size=int(rng.integers(6, 13)))]:
        e.new_worker(WB(c).res_sum("gpus", 2))
    st = dict(ticks=0, starts=0, from_prefill=0, disposals=0, lost_pf=0, lost=0, drawn=0, skipped=0)
    n_msgs, level = 0, 0

    def new_msgs(ready=False):
        nonlocal n_msgs
        msgs = e.retract_messages[n_msgs:]; n_msgs = len(e.retract_messages)
        st["disposals"] += len(msgs)
        h.disposed(msgs, {t: (e.tasks[t].priority, e.tasks[t].rq) for (_, t) in msgs} if ready else None)

    try:
        for round_ in range(10):
            # new tasks of three user priorities; a higher-priority arrival dissolves the prefill sets below it (check_dispose_prefill)
            # (the level rises in two of the rounds only: between them the prefill sets live on, and the next ticks hand their tasks out as redirects)
            if round_ in (3, 7):
                level += 1
            for _ in range(int(rng.integers(4, 16)) if round_ else int(rng.integers(60, 90))):
                e.new_task(shapes[int(rng.integers(0, len(shapes)))].user_priority(int(rng.integers(0, level + 1))))
            snap = e.snapshot()
            h.upload(snap)
            new_msgs()
            h.check(e)
            snap = e.snapshot()
            try:
                want = h.b_tick(snap)
            except HqTickError as err:
                assert err.code == abi.HQTICK_E_UNSUPPORTED
                break
            except RuntimeError as err:  # (the oracle's form of the same refusal)
                assert "failed: -6" in str(err)
                break
            h.tick(snap, want)
            e.apply(want)
            st["ticks"] += 1
            st["from_prefill"] += sum(1 for k in (want.redirect_kinds or []) if k == abi.HQ_REDIRECT_FROM_PREFILL)
            h.check(e)
            # prefilled tasks start on their workers (task_from_prefilled_to_started), one batch
            pairs = []
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state == PREFILLED and rng.random() < 0.3:
                    v = int(rng.integers(0, len(e.requests[t.rq])))
                    e.start_prefilled_task(t.id, v); pairs.append((t.id, v))
            if pairs:
                h.started(pairs); st["starts"] += len(pairs)
                h.check(e)
            # finishes
            batch = []
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state in (ASSIGNED, RUNNING) and rng.random() < 0.4:
                    e.finish_task(t.id, t.worker); batch.append(t.id)
            h.released(batch)
            h.check(e)
            # cancels and rejects of prefilled tasks (reactor.rs:762-766, :406-413)
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state == PREFILLED and rng.random() < 0.1:
                    st["disposals"] += 1
                    if rng.random() < 0.5:
                        e.cancel_prefilled_task(t.id)
                        h.unprefilled([t.id])
                    else:
                        wid = t.worker
                        e.reject_task(t.id, wid, 0)
                        h.unprefilled([t.id])
                        h.blocked(wid, sorted(e.workers[wid].blocked_requests))
                        new_msgs()
                    h.check(e)
            # the workers answer some retracts (not of tasks a tick put back on the worker they are retracting from: no redirect, mapping.rs:69)
            for t in [t for t in sorted(e.tasks.values(), key=lambda t: t.id) if t.state == RETRACTING and t.id not in e.retaken_variant][:6]:
                if rng.random() < 0.9:
                    expect = [(t.id,) + tuple(e.redirects[t.id])] if t.id in e.redirects else []
                    wid = t.worker
                    e.retract_response(wid, [t.id])
                    h.response(wid, [t.id], expect)
            h.check(e)
            # a worker joins
            if rng.random() < 0.4:
                wid = e.new_worker(WB(int(rng.integers(2, 6))).res_sum("gpus", 2))
                s2 = e.snapshot(); i = s2.worker_id.tolist().index(wid)
                tot = np.asarray(s2.worker_total, np.uint64).reshape(len(s2.worker_id), s2.n_resources)[i:i + 1]
                h.joined(wid, tot)
                h.check(e)
            # a worker is lost; every other draw prefers one that holds prefilled tasks
            if len(e.workers) > 4 and st["lost"] < 4 and rng.random() < 0.7:
                ok = [w for w, x in sorted(e.workers.items())
                      if not any(e.tasks[t].state == RETRACTING and t not in e.redirects for t in x.assigned_tasks)]  # (remove_worker wants a redirect to drop)
                with_pf = [w for w in ok if e.workers[w].prefilled_tasks]
                pool = with_pf if (with_pf and (seed + round_) % 2 == 0) else ok
                if pool:
                    st["drawn"] += 1
                    wid = pool[int(rng.integers(0, len(pool)))]
                    x = e.workers[wid]
                    live = [p for (p, s) in e.prefill.values() if len(s)]
                    # a worker that holds prefilled tasks is lost only when every assigned task on it has a priority no higher than every live prefill set's:
                    # otherwise re-adding the assigned task dissolves a set first (check_dispose_prefill) and the reference itself panics when
                    # move_prefilled_task_to_ready then looks for the prefilled task in it (taskqueue.rs:264)
                    if x.prefilled_tasks and any(e.tasks[t].priority > p for t in x.assigned_tasks for p in live):
                        st["skipped"] += 1
                    else:
                        h.before_loss(e.snapshot())
                        pf_back = sorted(x.prefilled_tasks)
                        back = [(t, e.tasks[t].rq, e.tasks[t].priority) for t in sorted(set(x.assigned_tasks) | set(x.prefilled_tasks))]
                        sent = e.remove_worker(wid)
                        h.lost(wid, sent, back, pf_back)
                        st["lost"] += 1; st["lost_pf"] += 1 if pf_back else 0
                        new_msgs(ready=True)  # the re-added tasks may dissolve prefill sets of the workers that stay
                        h.ready_is(len(e.snapshot().task_id))
                        h.check(e)
        assert st["ticks"] >= 2, st
    finally:
        h.close()
    _STATS[seed] = st
    return st


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_ledger_follows_sched_env_with_prefilled_tasks(seed):
    _scenario(seed)


def test_the_scenarios_cover_starts_redirects_disposals_and_losses():
    for seed in range(N_SEEDS):  # (a run that selected only this test plays the scenarios itself)
        if seed not in _STATS:
            _scenario(seed)
    tot = {k: sum(s[k] for s in _STATS.values()) for k in next(iter(_STATS.values()))}
    assert tot["starts"] >= 30 and tot["from_prefill"] >= 10 and tot["disposals"] >= 10 and tot["lost_pf"] >= 5, tot
    assert tot["skipped"] * 4 <= tot["drawn"], tot


# ---------------------------------------------------------------------------------------------- 3: rows across wavefront boundaries
PF_ROWS = [[0, 63, 64], [65, 129], [1, 2, 3, 127, 128]]


def _make_prefilled(e, builder, wid):
    """a task in state Prefilled{wid} (what a tick's PREFILL record leaves behind, core.py: apply)"""
    from hyperqueue_amd.hbmap import task_id_set

    tid = e.new_task(builder)
    t = e.tasks[tid]
    t.state, t.worker = PREFILLED, wid
    e.workers[wid].prefilled_tasks.add(tid)
    e.ready[t.rq].discard(tid)
    if t.rq not in e.prefill or len(e.prefill[t.rq][1]) == 0:
        e.prefill[t.rq] = (t.priority, task_id_set())
    e.prefill[t.rq][1].insert(tid)
    return tid


def _wide_env():
    """130 workers (rows = id - 50); running tasks on rows outside PF_ROWS; per group of PF_ROWS prefilled tasks of one shape, an AMOUNT and an ALL request
    together on every row"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

    e = SchedEnv(abi.make_config(fill_max=2, time_limit_s=20.0))
    gpu = e.new_named_resource("gpus")
    wids = e.new_workers(130, WB(8).res_sum("gpus", 2))
    assert wids == list(range(50, 180))
    for row in (4, 10, 62, 66, 100, 126):
        e.new_task_running(TB().cpus(1), wids[row]); e.new_task_running(TB().cpus(1).add_resource(gpu, 1), wids[row])
    group_shapes = [[TB().cpus(1), TB().cpus_all()], [TB().cpus(2).add_all(gpu), TB().cpus(1)], [TB().cpus(3).next_variant().cpus(1), TB().add_resource(gpu, 0.5)]]
    pf = []
    for rows, shapes in zip(PF_ROWS, group_shapes):
        for r in rows:
            for s in shapes:
                pf.append(_make_prefilled(e, s, wids[r])); pf.append(_make_prefilled(e, s, wids[r]))
    pf.append(_make_prefilled(e, TB().cpus(1), wids[10]))  # a busy row holds one too
    return e, wids, pf


def _wide_ctx(e):
    from hyperqueue_amd.tick import Tick

    t = Tick(abi.make_config(fill_max=2, time_limit_s=20.0))
    t.cluster_upload(e.snapshot())
    tasks = sorted(e.tasks.values(), key=lambda x: x.id)
    t.assigned_enable([(x.id, x.worker, x.rq, x.rv, x.priority) for x in tasks if x.state == RUNNING])
    seed = [(x.id, x.worker, x.rq, x.priority) for x in tasks if x.state == PREFILLED]
    assert t.assigned_track_prefilled(seed) == len(seed) and t.assigned_last_unknown() == 0
    return t


def test_one_start_batch_in_three_orders_leaves_the_same_rows_and_counts():
    views = []
    for order in ("forward", "reverse", "interleaved"):
        e, wids, pf = _wide_env()
        t = _wide_ctx(e)
        try:
            _check_state(e, t)
            some = pf[::2] + pf[1::4]  # both tasks of some (row, shape) pairs, one of the others
            batch = {"forward": some, "reverse": some[::-1], "interleaved": some[1::2] + some[::2]}[order]
            pairs = [(tid, 1 if len(e.requests[e.tasks[tid].rq]) > 1 and tid % 2 else 0) for tid in batch]
            for tid, v in pairs:
                e.start_prefilled_task(tid, v)
            assert t.assigned_start_prefilled(pairs) == len(pairs) and t.assigned_last_unknown() == 0
            _check_state(e, t)
            views.append(_view(t, sorted(e.tasks)))
        finally:
            t.close()
    assert views[0] == views[1] == views[2]


def test_a_worker_with_and_one_without_prefilled_tasks_lost_in_one_call_in_either_order():
    states = []
    for ids in ([114, 116], [116, 114]):  # rows 64 (prefilled tasks only) and 66 (running tasks only)
        e, wids, pf = _wide_env()
        t = _wide_ctx(e)
        try:
            snap = e.snapshot()
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
            back, pf_back = [], []
            for wid in ids:
                x = e.workers[wid]
                back += [(y, e.tasks[y].rq, e.tasks[y].priority) for y in set(x.assigned_tasks) | set(x.prefilled_tasks)]
                pf_back += list(x.prefilled_tasks)
                assert e.remove_worker(wid) == []
            assert len(pf_back) == 4 and len(back) == 6
            assert t.cluster_remove_workers(ids) == []
            assert t.cluster_last_requeued() == sorted(back)
            assert t.cluster_last_requeued_prefilled() == sorted(pf_back)
            assert t.ready_count() == len(e.snapshot().task_id)
            _check_state(e, t)
            states.append(_view(t, sorted(e.tasks)))
        finally:
            t.close()
    assert states[0] == states[1]


# ---------------------------------------------------------------------------------------------- 4: refusals
def test_refusals_are_counted_and_change_nothing():
    from hyperqueue_amd.tick import HqTickError, Tick

    cfg, e = _two_tick_env()
    a, b = Tick(cfg), Tick(cfg)
    try:
        snap = e.snapshot()
        a.cluster_upload(snap)
        with pytest.raises(HqTickError) as err:  # no ledger
            a.assigned_track_prefilled([])
        assert err.value.code == abi.HQTICK_E_INVALID
        a.assigned_enable([])
        for call in (lambda: a.assigned_start_prefilled([(1, 0)]), lambda: a.assigned_unprefill([1])):  # a ledger, but no tracking
            with pytest.raises(HqTickError) as err:
                call()
            assert err.value.code == abi.HQTICK_E_INVALID
        assert a.assigned_prefilled_count() == 0
        a.assigned_track_prefilled([])
        want = b.tick(_b_snap(snap))
        _same(_ledger_tick(a, snap), want)
        e.apply(want)
        ids = sorted(e.tasks)
        pf = [x for x in ids if e.tasks[x].state == PREFILLED]
        run = [x for x in ids if e.tasks[x].state == ASSIGNED]
        assert len(pf) == 8 and len(run) == 16
        before = _view(a, ids)
        # a snapshot that carries the prefilled CSR as well: two truths
        with pytest.raises(HqTickError) as err:
            _ledger_tick(a, e.snapshot(), prefilled_csr=True)
        assert err.value.code == abi.HQTICK_E_INVALID
        assert _view(a, ids) == before
        unknown = max(ids) + 1000
        assert a.assigned_start_prefilled([(unknown, 0)]) == 0 and a.assigned_last_unknown() == 1  # an unknown id
        assert a.assigned_start_prefilled([(run[0], 0)]) == 0 and a.assigned_last_unknown() == 1   # an assigned id
        assert a.assigned_start_prefilled([(pf[0], 1)]) == 0 and a.assigned_last_unknown() == 1    # a variant the request does not have
        assert a.assigned_start_prefilled([(pf[0], 0xFE)]) == 0 and a.assigned_last_unknown() == 1
        assert _view(a, ids) == before
        assert a.assigned_unprefill([run[0], unknown]) == 0 and a.assigned_last_unknown() == 2     # an assigned entry is never touched
        assert a.assigned_release([pf[0]]) == 0 and a.assigned_last_unknown() == 1                 # a prefilled task is not running
        t0 = e.tasks[pf[0]]
        assert a.assigned_add([(pf[0], t0.worker, t0.rq, 0, t0.priority)]) == 0 and a.assigned_last_unknown() == 1  # already present: a duplicate
        assert _view(a, ids) == before
        _check_state(e, a)
        # a good id beside the bad ones, and the same id twice in one batch
        e.start_prefilled_task(pf[1], 0)
        assert a.assigned_start_prefilled([(unknown, 0), (pf[1], 0), (pf[1], 0), (run[1], 0)]) == 1 and a.assigned_last_unknown() == 3
        e.cancel_prefilled_task(pf[2])
        assert a.assigned_unprefill([pf[2], pf[2], run[2]]) == 1 and a.assigned_last_unknown() == 2
        _check_state(e, a)
        # a second seed replaces the prefilled entries; refused entries are counted and enter nothing
        left = [x for x in pf if e.tasks[x].state == PREFILLED]
        wids = sorted(e.workers)
        seed = [(x, e.tasks[x].worker, e.tasks[x].rq, e.tasks[x].priority) for x in left]
        bad = [(unknown, 999, 0, 0), (unknown + 1, wids[0], 10_000, 0), (run[3], wids[0], 0, 0), seed[0]]  # an unknown worker, an unknown request, an id of the ledger, an id twice
        assert a.assigned_track_prefilled(seed + bad) == len(seed) and a.assigned_last_unknown() == 4
        _check_state(e, a)
    finally:
        a.close(); b.close()


def test_the_new_calls_wait_for_a_pending_placement():
    from hyperqueue_amd.tick import HqTickError, Tick

    cfg, e = _two_tick_env()
    snap = e.snapshot()
    a = Tick(cfg)
    try:
        a.cluster_upload(snap); a.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        a.assigned_enable([]); a.assigned_track_prefilled([])
        r = abi.parse_result(a.tick_raw(_strip(snap.to_c(resident_workers=True)), resident=True), len(snap.worker_id), snap.n_resources)
        pf = [x[0] for w in r.records for x in w if x[2] == abi.HQ_REC_PREFILL]
        assert len(pf) == 8 and a.assigned_prefilled_count() == 0  # pending until consumed
        for call in (lambda: a.assigned_track_prefilled([]), lambda: a.assigned_start_prefilled([(pf[0], 0)]), lambda: a.assigned_unprefill([pf[0]])):
            with pytest.raises(HqTickError) as err:
                call()
            assert err.value.code == abi.HQTICK_E_INVALID
        a.ready_consume_last()
        assert a.assigned_prefilled_count() == 8 and a.assigned_count() == 16
        assert a.assigned_start_prefilled([(pf[0], 0)]) == 1 and a.assigned_unprefill([pf[1]]) == 1
        assert a.assigned_prefilled_count() == 6 and a.assigned_count() == 17
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 5: record forms and consume forms
class _Env:
    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _resident_ctx(cfg, snap, form="plain", flags=0, ordered=False, sink_records=4096):
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import Tick
    from test_gpu_assigned_forms import Sink

    with _Env(**({"HQTICK_ORDERED_VIEW": "1"} if ordered else {})):
        t = Tick(abi.make_config(reserve=cfg.proactive_filling_reserve, fill_max=cfg.proactive_filling_max, time_limit_s=20.0, flags=flags | FORM_FLAGS[form]))
    t.cluster_upload(snap)
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    t.assigned_enable([]); t.assigned_track_prefilled([])
    return t, (Sink(t, sink_layout(len(snap.worker_id), sink_records)[4]) if form == "sink" else None)


def _resident_tick(t, snap, sink=None):
    from test_gpu_assigned_forms import _parse

    return _parse(t.tick_raw(_strip(snap.to_c(resident_workers=True)), resident=True), len(snap.worker_id), snap.n_resources, sink)


@pytest.mark.parametrize("ordered", [False, True], ids=["dense", "ordered_view"])
@pytest.mark.parametrize("flags,form", [(0, "plain"), (IN_TICK, "plain"), (0, "compact"), (IN_TICK, "compact"), (0, "delta16"), (IN_TICK, "delta16"), (0, "sink"), (IN_TICK, "sink")])
def test_the_two_ticks_in_every_consume_form_and_record_form(flags, form, ordered):
    from hyperqueue_amd.tick import Tick

    cfg, e = _two_tick_env()
    snap = e.snapshot()
    a, sink = _resident_ctx(cfg, snap, form, flags, ordered)
    b = Tick(cfg)
    try:
        want = b.tick(_b_snap(snap))
        got = _resident_tick(a, snap, sink)
        if not flags & IN_TICK:
            assert a.assigned_prefilled_count() == 0 and a.assigned_count() == 0
            a.ready_consume_last()
        _same(got, want)
        assert a.assigned_last_host_bytes() == 0
        e.apply(want)
        _check_state(e, a)
        done, new = _between_the_ticks(e)
        assert a.assigned_release(done) == len(done)
        a.ready_add(np.asarray(new, np.uint64), np.asarray([e.tasks[x].priority for x in new], np.uint64), np.asarray([e.tasks[x].rq for x in new], np.uint32))
        snap = e.snapshot()
        want = b.tick(_b_snap(snap))
        got = _resident_tick(a, snap, sink)
        if not flags & IN_TICK:
            a.ready_consume_last()
        _same(got, want)
        assert _n_kind(want, abi.HQ_REC_ASSIGN) == 4 and _n_kind(want, abi.HQ_REC_PREFILL) == 0
        assert a.assigned_last_host_bytes() == 0
        e.apply(want)
        _check_state(e, a)
    finally:
        a.close(); b.close()


def test_an_abandoned_two_call_tick_enters_no_prefilled_task():
    cfg, e = _two_tick_env()
    snap = e.snapshot()
    t, _ = _resident_ctx(cfg, snap)
    try:
        r = _resident_tick(t, snap)
        ids = sorted(x[0] for w in r.records for x in w)
        assert _n_kind(r, abi.HQ_REC_PREFILL) == 8
        top = int(snap.task_id.max()) + 1
        t.ready_add_packed([(top, 4)], [(int(snap.task_priority[0]), 4)], np.full(4, int(snap.task_rq[0]), np.uint16))  # a ready-set delta drops the tick's selection
        t.ready_consume_last()
        assert t.assigned_prefilled_count() == 0 and t.assigned_count() == 0
        assert (t.assigned_lookup(ids)[0] == abi.HQ_NO_WORKER).all()
        r2 = _resident_tick(t, snap)  # the next tick places them again, and this time the placement enters
        t.ready_consume_last()
        assert _n_kind(r2, abi.HQ_REC_PREFILL) == 8 and t.assigned_prefilled_count() == 8 and t.assigned_count() == 16
        pf = sorted(x[0] for w in r2.records for x in w if x[2] == abi.HQ_REC_PREFILL)
        assert t.assigned_lookup(pf)[1].tolist() == [PF] * 8
    finally:
        t.close()


def test_a_failing_consume_in_tick_tick_leaves_the_prefilled_entries_as_they_were():
    """CONSUME_IN_TICK with a sink sized for 8 records on a tick that produces more: HQTICK_E_CAPACITY, and prefilled count, lookups and free rows are untouched"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import HqTickError
    from test_gpu_assigned_forms import Sink

    cfg = abi.make_config(reserve=0, fill_max=2, time_limit_s=20.0)
    e = SchedEnv(cfg)
    e.new_workers_cpus([8] * 4)
    for _ in range(40):
        e.new_task(TB().cpus(1))
    snap = e.snapshot()
    W = len(snap.worker_id)
    a, big = _resident_ctx(cfg, snap, "sink", IN_TICK)
    try:
        r = _resident_tick(a, snap, big)
        e.apply(r)
        assert a.assigned_prefilled_count() == 8 and a.assigned_count() == 32
        done = [x for x in sorted(e.tasks) if e.tasks[x].state == ASSIGNED]
        for x in done:
            e.finish_task(x, e.tasks[x].worker)
        assert a.assigned_release(done) == 32  # 32 free cpus again: the next tick hands out the 8 prefilled tasks (redirects) and 24 records at least
        new = [e.new_task(TB().cpus(1)) for _ in range(40)]
        a.ready_add(np.asarray(new, np.uint64), np.asarray([e.tasks[x].priority for x in new], np.uint64), np.asarray([e.tasks[x].rq for x in new], np.uint32))
        _check_state(e, a)
        ids = sorted(e.tasks)
        live, before = a.ready_count(), _view(a, ids)
        small = Sink(a, sink_layout(W, 8)[4])
        assert small.capacity(W) <= 16
        with pytest.raises(HqTickError) as err:
            _resident_tick(a, e.snapshot(), small)
        assert err.value.code == abi.HQTICK_E_CAPACITY
        assert a.ready_count() == live and _view(a, ids) == before
        _check_state(e, a)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 6: tracking off
def test_a_ledger_that_never_asks_for_tracking_takes_the_prefilled_csr_as_before():
    from hyperqueue_amd.tick import Tick

    cfg, e = _two_tick_env()
    a, b = Tick(cfg), Tick(cfg)
    try:
        snap = e.snapshot()
        a.cluster_upload(snap); a.assigned_enable([])
        want = b.tick(_b_snap(snap))
        _same(_ledger_tick(a, snap, prefilled_csr=True), want)
        e.apply(want)
        assert a.assigned_prefilled_count() == 0 and a.assigned_count() == 16
        pf = [x for x in sorted(e.tasks) if e.tasks[x].state == PREFILLED]
        assert (a.assigned_lookup(pf)[0] == abi.HQ_NO_WORKER).all()  # PREFILL records are skipped, as before
        done, _ = _between_the_ticks(e)
        assert a.assigned_release(done) == len(done)
        snap = e.snapshot()
        want = b.tick(_b_snap(snap))
        assert _n_kind(want, abi.HQ_REC_ASSIGN) == 4 and _n_kind(want, abi.HQ_REC_PREFILL) == 0
        _same(_ledger_tick(a, snap, prefilled_csr=True), want)
    finally:
        a.close(); b.close()
