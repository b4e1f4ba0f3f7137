"""The assignment ledger in every form in which a tick's records leave the device: plain records, HQTICK_FLAG_COMPACT_RECORDS,
HQTICK_FLAG_COMPACT_DELTA16 and a device record sink.  The mapping kernel stages the ledger's entries in HBM beside the records, so the same ledger must
come out of all four, no record data may come back from the host (hqtick_assigned_last_host_bytes == 0), and a tick that is abandoned or fails must leave
the ledger as it was.  Context B always runs today's protocol without a ledger."""
import ctypes as C
import dataclasses
import os
import random

import numpy as np
import pytest

from hyperqueue_amd import abi

pytestmark = pytest.mark.gpu

ASSIGNED, RUNNING, PREFILLED, RETRACTING = 1, 2, 3, 4
COMPACT = abi.HQTICK_FLAG_COMPACT_RECORDS
DELTA16 = abi.HQTICK_FLAG_COMPACT_RECORDS | abi.HQTICK_FLAG_COMPACT_DELTA16
IN_TICK = abi.HQTICK_FLAG_CONSUME_IN_TICK
FORMS = ["plain", "compact", "delta16", "sink"]
FORM_FLAGS = {"plain": 0, "compact": COMPACT, "delta16": DELTA16, "sink": 0}
SINK_MAGIC = 0x48515354


class Sink:
    """a device tensor given to hqtick_set_record_sink, and its records read back (layout: include/hqtick.h)"""

    def __init__(self, t, n_bytes):
        import torch

        self.t, self.buf = t, torch.zeros(n_bytes, dtype=torch.uint8, device="cuda:0")
        t.set_record_sink(self.buf)

    def capacity(self, W):
        f = self.t._lib.hqtick_sink_capacity_records
        f.argtypes = [C.c_uint32, C.c_size_t]; f.restype = C.c_uint32
        return int(f(W, self.buf.numel()))

    def records(self, W):
        from hyperqueue_amd.sharded import sink_layout

        h = self.buf.cpu().numpy()
        n, _chk, magic, cap = [int(x) for x in h[:16].view(np.uint32)]
        assert magic == SINK_MAGIC and cap == self.capacity(W) and n <= cap
        o_off, o_task, o_var, o_kind, _ = sink_layout(W, cap)
        off = h[o_off:o_off + (W + 1) * 4].view(np.uint32)
        assert int(off[W]) == n
        t = h[o_task:o_task + n * 8].view(np.uint64).tolist(); v = h[o_var:o_var + n].tolist(); k = h[o_kind:o_kind + n].tolist()
        return [list(zip(t[int(off[w]):int(off[w + 1])], v[int(off[w]):int(off[w + 1])], k[int(off[w]):int(off[w + 1])])) for w in range(W)]


def _parse(rc, W, R, sink=None):
    """the result of a tick; with a sink the records are not in the result (rec_task == NULL): they are read from the device tensor"""
    if sink is None:
        return abi.parse_result(rc, W, R)
    assert not rc.rec_task and not rc.rec_task_lo and not rc.rec_delta16
    n = int(np.ctypeslib.as_array(rc.rec_off, shape=(W + 1,))[W]) if W else 0
    keep = rc.rec_off
    rc.rec_off = None
    res = abi.parse_result(rc, W, R)
    rc.rec_off = keep
    recs = sink.records(W)
    assert sum(len(r) for r in recs) == n
    return dataclasses.replace(res, records=recs)


def _same(a, b):
    assert a.status == b.status and a.is_optimal == b.is_optimal and a.batches == b.batches
    assert a.counts == b.counts and a.records == b.records and a.retracts == b.retracts
    assert (a.new_free == b.new_free).all()
    assert a.redirects == b.redirects and a.redirect_kinds == b.redirect_kinds


def _ledger_tick(t, snap, sink=None):
    """a tick of a ledger context: resident workers, resident Retracting table, NO assigned CSR"""
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None
    sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
    return _parse(t.tick_raw(sc), len(snap.worker_id), snap.n_resources, sink)


def _check_state(e, t):
    snap = e.snapshot()
    assert t.cluster_workers().tolist() == sorted(e.workers)
    assert (t.assigned_free_rows() == np.asarray(snap.worker_free, np.uint64).reshape(len(snap.worker_id), snap.n_resources)).all()
    ids = sorted(e.tasks)
    w, _ = t.assigned_lookup(ids)
    got = {}
    for tid, wid in zip(ids, w.tolist()):
        if wid != abi.HQ_NO_WORKER:
            got.setdefault(wid, set()).add(tid)
    want = {wid: set(x.assigned_tasks) for wid, x in e.workers.items() if x.assigned_tasks}
    assert got == want
    assert t.assigned_count() == sum(len(x) for x in want.values())


def _start_prefilled(e, tid):
    """SchedEnv has no task_from_prefilled_to_started: the task leaves its prefill set and runs on its worker with variant 0 (insert_sn_task)"""
    t = e.tasks[tid]
    w = e.workers[t.worker]
    w.prefilled_tasks.discard(tid)
    e.prefill[t.rq][1].remove(tid)
    t.state, t.rv = RUNNING, 0
    e._remove(w, t.rq, 0)
    w.assigned_tasks.add(tid)


@pytest.mark.parametrize("seed", range(40))
def test_ledger_follows_sched_env_in_every_form(seed):
    """the event stream of test_gpu_assigned.py::test_ledger_follows_sched_env on four ledger contexts (plain, compact, delta16, plain + sink) and B"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import HqTickError, Tick

    rng = np.random.default_rng(31_000 + seed)
    kw = dict(reserve=int(rng.integers(0, 2)), fill_max=int(rng.integers(1, 4)), time_limit_s=20.0)
    cfg = abi.make_config(**kw)
    e = SchedEnv(cfg)
    b = Tick(cfg)
    led = {f: Tick(abi.make_config(flags=FORM_FLAGS[f], **kw)) for f in FORMS}
    sink = Sink(led["sink"], 1 << 18)  # (set before hqtick_assigned_enable here; after it in the tests below)
    sinks = {f: (sink if f == "sink" else None) for f in FORMS}
    ticks = {f: 0 for f in FORMS}
    gpu = e.new_named_resource("gpus")
    shapes = [TB().cpus(1), TB().cpus(2), TB().cpus_all(), TB().cpus(0.5), TB().cpus(3).next_variant().cpus(1),
              TB().cpus(1).add_resource(gpu, 1), TB().cpus(1).add_all(gpu), TB().add_resource(gpu, 0.5)]
    for c in [int(x) for x in np.random.default_rng(seed).integers(2, 6, size=4)]:
        e.new_worker(WB(c).res_sum("gpus", 2))
    prio, n_msgs, removed, uploaded = 0, 0, 0, False

    def retracting(msgs):
        for a in led.values():
            a.retracting_add([t for (_, t) in msgs], [w for (w, _) in msgs])

    def check_all():
        for a in led.values():
            _check_state(e, a)

    try:
        for round_ in range(8):
            for _ in range(int(rng.integers(1, 7)) if round_ else int(rng.integers(8, 16))):
                e.new_task(shapes[int(rng.integers(0, len(shapes)))].user_priority(prio))
            if rng.random() < 0.6:
                prio += 1
            new_msgs = e.retract_messages[n_msgs:]; n_msgs = len(e.retract_messages)
            if new_msgs and uploaded:
                retracting(new_msgs)
            snap = e.snapshot()
            if not uploaded:
                for a in led.values():
                    a.cluster_upload(snap); a.assigned_enable([])
                uploaded = True
                if new_msgs:
                    retracting(new_msgs)
            try:
                want = b.tick(dataclasses.replace(snap, worker_map_rank=None, _keep=[]))
            except HqTickError as err:
                assert err.code == abi.HQTICK_E_UNSUPPORTED
                break
            for f, a in led.items():
                _same(_ledger_tick(a, snap, sinks[f]), want)
                assert a.assigned_last_host_bytes() == 0
                ticks[f] += 1
            e.apply(want)
            check_all()
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state == PREFILLED and rng.random() < 0.3:
                    _start_prefilled(e, t.id)
                    for a in led.values():
                        assert a.assigned_add([(t.id, t.worker, t.rq, 0, t.priority)]) == 1 and a.assigned_last_unknown() == 0
            check_all()
            batch = []
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state in (ASSIGNED, RUNNING) and rng.random() < 0.35:
                    if t.state == ASSIGNED and rng.random() < 0.25:
                        wid, v = t.worker, t.rv
                        e.reject_task(t.id, wid, v)
                        for a in led.values():
                            a.cluster_set_blocked(wid, sorted(e.workers[wid].blocked_requests))
                    else:
                        e.finish_task(t.id, t.worker)
                    batch.append(t.id)
            for a in led.values():
                assert a.assigned_release(batch[:]) == len(batch) and a.assigned_last_unknown() == 0
            new_msgs = e.retract_messages[n_msgs:]; n_msgs = len(e.retract_messages)
            if new_msgs:
                retracting(new_msgs)
            check_all()
            if rng.random() < 0.3:
                wid = e.new_worker(WB(int(rng.integers(2, 6))))
                s2 = e.snapshot(); i = s2.worker_id.tolist().index(wid)
                tot = np.asarray(s2.worker_total, np.uint64).reshape(len(s2.worker_id), s2.n_resources)[i:i + 1]
                for a in led.values():
                    a.cluster_add_workers([wid], tot, tot)
                check_all()
            busy = [w for w, x in sorted(e.workers.items()) if x.assigned_tasks]
            if busy and len(e.workers) > 2 and removed < 2 and rng.random() < 0.5:
                wid = busy[int(rng.integers(0, len(busy)))]
                if any(e.tasks[x].state == RETRACTING and x not in e.redirects for x in e.workers[wid].assigned_tasks):
                    continue
                if e.workers[wid].prefilled_tasks:
                    continue
                back = sorted(e.workers[wid].assigned_tasks)
                sent = e.remove_worker(wid)
                for a in led.values():
                    assert a.cluster_remove_workers([wid]) == sent
                    assert a.cluster_last_requeued() == [(t, e.tasks[t].rq, e.tasks[t].priority) for t in back]
                removed += 1
                new_msgs = e.retract_messages[n_msgs:]; n_msgs = len(e.retract_messages)
                if new_msgs:
                    retracting(new_msgs)
                check_all()
            for a in led.values():
                assert a.retracting_count() == sum(1 for t in e.tasks.values() if t.state == RETRACTING)
        # every form compared as many ticks as the plain ledger context (B's refusal ends all of them on the same tick), and at least one
        assert all(ticks[f] == ticks["plain"] for f in FORMS) and ticks["plain"] >= 1, ticks
    finally:
        b.close()
        for a in led.values():
            a.close()


def _steady_snap(n_tasks, n_workers, seed, name="c3"):
    from hyperqueue_amd import workloads

    snap = workloads.make_steady(name, seed=seed, n_tasks=n_tasks, n_workers=n_workers)
    return dataclasses.replace(snap, assigned=[[] for _ in snap.worker_id], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])


def _resident_ctx(snap, form, flags=0, env=None, ledger=True, sink_records=None):
    """a context with resident workers and ready set; the ledger on; form "sink": the sink is set AFTER the ledger was enabled"""
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import Tick

    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        t = Tick(abi.make_config(time_limit_s=20.0, flags=flags | FORM_FLAGS[form]))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    t.cluster_upload(snap)
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    if ledger:
        t.assigned_enable([])
    sink = None
    if form == "sink":
        W = len(snap.worker_id)
        sink = Sink(t, sink_layout(W, sink_records if sink_records is not None else len(snap.task_id))[4])
    return t, sink


def _resident_tick(t, snap, sink=None):
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    return _parse(t.tick_raw(sc, resident=True), len(snap.worker_id), snap.n_resources, sink)


def _n_assign(res):
    return sum(1 for w in res.records for r in w if r[2] == abi.HQ_REC_ASSIGN)


def _ledger_view(t, ids):
    return t.assigned_count(), t.assigned_free_rows().tolist(), [a.tolist() for a in t.assigned_lookup(ids)]


@pytest.mark.parametrize("form", ["compact", "delta16", "sink"])
def test_consume_forms_and_scan_paths_feed_the_same_ledger(form):
    """two-call form, CONSUME_IN_TICK and the ordered view (HQTICK_ORDERED_VIEW=1) in one emission form: same records, same ledger"""
    snap = _steady_snap(60_000, 64, 7)
    ctxs = [_resident_ctx(snap, form), _resident_ctx(snap, form, IN_TICK), _resident_ctx(snap, form, IN_TICK, env={"HQTICK_ORDERED_VIEW": "1"})]
    try:
        for _ in range(3):
            res = []
            for i, (t, sink) in enumerate(ctxs):
                res.append(_resident_tick(t, snap, sink))
                if i == 0:
                    t.ready_consume_last()
                assert t.assigned_last_host_bytes() == 0
            assert res[0].records == res[1].records == res[2].records and _n_assign(res[0]) > 0
            ids = sorted(r[0] for w in res[0].records for r in w)
            views = [_ledger_view(t, ids) for t, _ in ctxs]
            assert views[0] == views[1] == views[2]
            assert views[0][1] == res[0].new_free.tolist()
            placed = {r[0]: (int(snap.worker_id[w]), r[1]) for w, recs in enumerate(res[0].records) for r in recs if r[2] == abi.HQ_REC_ASSIGN}
            wids, vs = views[0][2]
            for tid, wid, v in zip(ids, wids, vs):
                assert (wid, v) == placed.get(tid, (abi.HQ_NO_WORKER, 0xFF))
            run = [r[0] for w in res[0].records for r in w if r[2] == abi.HQ_REC_ASSIGN][::2]
            for t, _ in ctxs:
                assert t.assigned_release(run) == len(run)
            assert ctxs[0][0].assigned_free_rows().tolist() == ctxs[1][0].assigned_free_rows().tolist() == ctxs[2][0].assigned_free_rows().tolist()
    finally:
        for t, _ in ctxs:
            t.close()


@pytest.mark.parametrize("in_tick", [False, True], ids=["two_call", "consume_in_tick"])
@pytest.mark.parametrize("form", FORMS)
def test_records_stay_on_the_device(form, in_tick):
    """60 000 tasks, 64 workers: nothing of the records is copied from the host when the placement enters the ledger"""
    snap = _steady_snap(60_000, 64, 7)
    t, sink = _resident_ctx(snap, form, IN_TICK if in_tick else 0)
    try:
        for _ in range(2):
            before = t.assigned_count()
            r = _resident_tick(t, snap, sink)
            if not in_tick:
                assert t.assigned_count() == before  # pending until consumed
                t.ready_consume_last()
            n = _n_assign(r)
            assert n > 0 and t.assigned_count() == before + n
            assert t.assigned_last_host_bytes() == 0
            assert (t.assigned_free_rows() == r.new_free).all()
            run = [x[0] for w in r.records for x in w if x[2] == abi.HQ_REC_ASSIGN]
            assert t.assigned_release(run) == n  # (the workers are free again for the next tick)
    finally:
        t.close()


@pytest.mark.parametrize("form", ["sink", "compact"])
def test_an_abandoned_two_call_tick_never_enters_the_ledger(form):
    snap = _steady_snap(40_000, 32, 9)
    a, sink = _resident_ctx(snap, form)
    b, _ = _resident_ctx(snap, "plain", ledger=False)
    try:
        free0 = a.assigned_free_rows()
        r = _resident_tick(a, snap, sink)
        ids = sorted(x[0] for w in r.records for x in w)
        assert _n_assign(r) > 0
        top = int(snap.task_id.max()) + 1
        for t in (a, b):
            t.ready_add_packed([(top, 16)], [(0, 16)], np.zeros(16, np.uint16))
        live = a.ready_count()
        a.ready_consume_last()
        assert a.ready_count() == live and a.assigned_count() == 0
        assert (a.assigned_free_rows() == free0).all()
        assert (a.assigned_lookup(ids)[0] == abi.HQ_NO_WORKER).all()
        assert a.assigned_release([top]) == 0 and a.assigned_last_unknown() == 1
        # the next tick equals B's (same ready set, free workers), and this time its placement enters
        r2 = _resident_tick(a, snap, sink)
        a.ready_consume_last()
        rb = abi.parse_result(b.tick_raw(snap.to_c(resident_workers=True), resident=True), len(snap.worker_id), snap.n_resources)
        _same(r2, rb)
        assert _n_assign(r2) > 0 and a.assigned_count() == _n_assign(r2) and (a.assigned_free_rows() == r2.new_free).all()
    finally:
        a.close(); b.close()


def test_a_sink_too_small_fails_the_tick_and_leaves_the_ledger_as_it_was():
    """CONSUME_IN_TICK with a sink sized for fewer records than the tick produces: HQTICK_E_CAPACITY (an error path the library defines), the ready set
    restored, the ledger, the counts and the free rows untouched; the same tick with a large enough sink equals B's"""
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import HqTickError

    snap = _steady_snap(40_000, 32, 9)
    W, R = len(snap.worker_id), snap.n_resources
    a, _ = _resident_ctx(snap, "plain", IN_TICK)
    b, _ = _resident_ctx(snap, "plain", IN_TICK, ledger=False)
    try:
        # one good tick first, so that the ledger, the count table and the free rows are not empty when the failing tick comes
        big = Sink(a, sink_layout(W, len(snap.task_id))[4])
        r0 = _resident_tick(a, snap, big)
        rb0 = abi.parse_result(b.tick_raw(snap.to_c(resident_workers=True), resident=True), W, R)
        _same(r0, rb0)
        keep = [x[0] for w in r0.records for x in w if x[2] == abi.HQ_REC_ASSIGN]
        gone = keep[::2]
        assert a.assigned_release(gone) == len(gone)
        ent = [[[(int(r), int(k), int(am)) for (r, k, am) in v["entries"]] for v in rq] for rq in snap.requests]
        rq_of = dict(zip(snap.task_id.tolist(), snap.task_rq.tolist()))
        free = np.asarray(rb0.new_free, np.uint64).reshape(W, R).copy()
        total = np.asarray(snap.worker_total, np.uint64).reshape(W, R)
        where = {x[0]: (w, x[1]) for w, recs in enumerate(r0.records) for x in recs if x[2] == abi.HQ_REC_ASSIGN}
        for tid in gone:
            w, v = where[tid]
            for (res, kind, amount) in ent[rq_of[tid]][v]:
                free[w, res] = total[w, res] if kind == abi.HQ_ENTRY_ALL else free[w, res] + np.uint64(amount)
        assert (a.assigned_free_rows() == free).all()
        b.cluster_update_workers(list(range(W)), free)
        per_w = [[(rq_of[x[0]], x[1]) for x in r0.records[w] if x[2] == abi.HQ_REC_ASSIGN and x[0] not in set(gone)] for w in range(W)]
        sb = dataclasses.replace(snap, assigned=per_w, worker_free=free.copy(), _keep=[])
        ids = sorted(where)
        live, before = a.ready_count(), _ledger_view(a, ids)
        small = Sink(a, sink_layout(W, 8)[4])
        assert small.capacity(W) < 64
        with pytest.raises(HqTickError) as err:
            _resident_tick(a, snap, small)
        assert err.value.code == abi.HQTICK_E_CAPACITY
        assert a.ready_count() == live and _ledger_view(a, ids) == before
        # the count-derived state: the next tick reads the per-worker (rq, variant) counts from the ledger and must place as B does from its CSR
        big2 = Sink(a, sink_layout(W, len(snap.task_id))[4])
        r1 = _resident_tick(a, snap, big2)
        rb1 = abi.parse_result(b.tick_raw(sb.to_c(resident_workers=True), resident=True), W, R)
        _same(r1, rb1)
        assert _n_assign(r1) > 0 and a.assigned_count() == before[0] + _n_assign(r1) and (a.assigned_free_rows() == r1.new_free).all()
        # the sink is removed again between ticks: the records come back in the result
        a.set_record_sink(None)
        r2 = _resident_tick(a, snap)
        assert a.assigned_count() == before[0] + _n_assign(r1) + _n_assign(r2)
    finally:
        a.close(); b.close()


def test_tick_to_bytes_with_the_ledger_on():
    """the scenario of test_zz_gpu_wire.py::test_tick_to_bytes_through_the_record_sink on a plain Tick with resident workers, the ledger and a sink: the
    tick's records stay in HBM, feed the ledger there and are encoded there"""
    import wire_cases as wc
    from hyperqueue_amd import wire
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import Tick
    from oracle.oracle import Oracle

    env = SchedEnv()
    env.new_named_resource("gpus/amd")
    env.new_workers(6, WB(16).res_sum("gpus/amd", 2))
    env.new_tasks(200, TB().cpus(1))
    env.new_tasks(40, TB().cpus(4).user_priority(1))
    env.new_tasks(30, TB().cpus(2).add_resource(1, 0.5))
    snap = env.snapshot()
    want = Oracle(env.config, canonical=True).tick(snap)
    W, R, cap = len(snap.worker_id), snap.n_resources, 4096
    t = Tick(env.config)
    try:
        t.cluster_upload(snap)
        t.assigned_enable([])
        sink = Sink(t, sink_layout(W, cap)[4])
        assert sink.capacity(W) == cap
        sc = snap.to_c(resident_workers=True)
        sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
        res_c = t.tick_raw(sc)
        n_records = int(np.ctypeslib.as_array(res_c.rec_off, shape=(W + 1,))[W])
        assert n_records == sum(len(r) for r in want.records) > 0
        assert t.assigned_last_host_bytes() == 0
        rnd = random.Random(9)
        configs = [(None, b"prog-a" * 30), ((600, 0), b"prog-b" * 70), ((5, 250), b"")]
        attrs = {x: (rnd.randrange(4), rnd.randrange(50), (0x80000000 + rnd.randrange(3)) << 32, rnd.randrange(3), None if rnd.random() < 0.6 else b"e-%d" % (x & 0xFFFF))
                 for recs in want.records for (x, v, k) in recs}
        worker_ids = [int(w) for w in snap.worker_id]
        scen = (attrs, configs, worker_ids, want.records, want.retracts, [])
        tables, side = wc.tables_and_records(*scen)
        got = wire.encode_from_sink(tables, sink.buf, W, cap, n_records, side, 1 << 22)
        assert got.status == wire.HQWIRE_OK and (got.slot_status == 0).all()
        assert got.messages(side) == wc.oracle_messages(*scen)
        # the ledger names, for every ASSIGN record of the oracle's result, the worker and variant the oracle gave it
        placed = [(x, worker_ids[w], v) for w, recs in enumerate(want.records) for (x, v, k) in recs if k == abi.HQ_REC_ASSIGN]
        assert placed and t.assigned_count() == len(placed)
        wids, vs = t.assigned_lookup([p[0] for p in placed])
        assert wids.tolist() == [p[1] for p in placed] and vs.tolist() == [p[2] for p in placed]
        assert (t.assigned_free_rows() == want.new_free).all()
        assert t.assigned_release([p[0] for p in placed]) == len(placed) and t.assigned_count() == 0
        assert (t.assigned_free_rows() == np.asarray(snap.worker_total, np.uint64).reshape(W, R)).all()
    finally:
        t.close()


def _entries(snap):
    return [[[(int(r), int(k), int(a)) for (r, k, a) in v["entries"]] for v in rq] for rq in snap.requests]


@pytest.mark.parametrize("form", ["sink", "delta16"])
def test_resident_loop_at_c3p_scale_matches_the_row_delta_protocol(form):
    """the 1 M-task, 1024-worker, 20-step loop of test_gpu_assigned.py with the ledger context in sink and in delta16 form: every step equal to B's"""
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import Tick

    snap = _steady_snap(1_000_000, 1024, 3, name="c3p")
    W, R = len(snap.worker_id), snap.n_resources
    a = Tick(abi.make_config(time_limit_s=20.0, flags=IN_TICK | FORM_FLAGS[form]))
    b = Tick(abi.make_config(time_limit_s=20.0, flags=IN_TICK))
    try:
        for t in (a, b):
            t.cluster_upload(snap); t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        a.assigned_enable([])
        sink = Sink(a, sink_layout(W, 1 << 18)[4]) if form == "sink" else None
        running = {}
        total = np.asarray(snap.worker_total, np.uint64).reshape(W, R)
        free = total.copy()
        rq_of = dict(zip(snap.task_id.tolist(), snap.task_rq.tolist()))
        ent = _entries(snap)
        prev = []
        next_id = int(snap.task_id.max()) + 1
        for step in range(20):
            if step:
                add = np.arange(next_id, next_id + 20_000, dtype=np.uint64); next_id += 20_000
                prio = np.zeros(len(add), np.uint64); rqs = (np.arange(len(add)) % len(snap.requests)).astype(np.uint32)
                for t in (a, b):
                    t.ready_add(add, prio, rqs)
                rq_of.update(zip(add.tolist(), rqs.tolist()))
            per_w = [[] for _ in range(W)]
            for tid, (w, q, v) in running.items():
                per_w[w].append((q, v))
            sb = dataclasses.replace(snap, assigned=per_w, worker_free=free.copy(), _keep=[])
            ra = _resident_tick(a, snap, sink)
            assert a.assigned_last_host_bytes() == 0
            rb = abi.parse_result(b.tick_raw(sb.to_c(resident_workers=True), resident=True), W, R)
            assert ra.records == rb.records and ra.counts == rb.counts and (ra.new_free == rb.new_free).all()
            nf = np.asarray(rb.new_free, np.uint64).reshape(W, R)
            changed = np.nonzero((nf != free).any(axis=1))[0].tolist()
            free = nf.copy()
            if changed:
                b.cluster_update_workers(changed, free[changed])
            new = []
            for w, recs in enumerate(rb.records):
                for (tid, v, kind) in recs:
                    if kind == abi.HQ_REC_ASSIGN:
                        running[tid] = (w, rq_of[tid], v); new.append(tid)
            assert a.assigned_count() == len(running)
            if prev:
                assert a.assigned_release(prev) == len(prev)
                touched = set()
                for tid in prev:
                    w, q, v = running.pop(tid)
                    for (res, kind, amount) in ent[q][v]:
                        free[w, res] = total[w, res] if kind == abi.HQ_ENTRY_ALL else free[w, res] + np.uint64(amount)
                    touched.add(w)
                idx = sorted(touched)
                b.cluster_update_workers(idx, free[idx])
                assert (a.assigned_free_rows() == free).all()
            prev = new
    finally:
        a.close(); b.close()
