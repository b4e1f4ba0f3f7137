"""Assignment ledger (hqtick_assigned_*, ABI 12): each worker's SingleNodeTaskAssignment kept by the library on the resident worker set.
Context A keeps the ledger (no row deltas for task starts / finishes, no assigned CSR); context B runs today's protocol on SchedEnv's full snapshot.
Every tick of A equals B's, and after every event A's free rows and per-worker tasks equal SchedEnv's."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from hyperqueue_amd import abi

pytestmark = pytest.mark.gpu

ASSIGNED, RUNNING, PREFILLED, RETRACTING = 1, 2, 3, 4


def _same(a, b):
    assert a.status == b.status and a.is_optimal == b.is_optimal and a.batches == b.batches
    assert a.counts == b.counts and a.records == b.records and a.retracts == b.retracts
    assert (a.new_free == b.new_free).all()
    assert a.redirects == b.redirects and a.redirect_kinds == b.redirect_kinds


def _ledger_tick(t, snap):
    """a tick of the ledger context: resident workers, resident Retracting table, NO assigned CSR"""
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None
    sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
    return abi.parse_result(t.tick_raw(sc), len(snap.worker_id), snap.n_resources)


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


@pytest.mark.parametrize("seed", range(40))
def test_ledger_follows_sched_env(seed):
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import HqTickError, Tick

    rng = np.random.default_rng(31_000 + seed)
    cfg = abi.make_config(reserve=int(rng.integers(0, 2)), fill_max=int(rng.integers(1, 4)), time_limit_s=20.0)
    e = SchedEnv(cfg)
    b, a = Tick(cfg), Tick(cfg)
    gpu = e.new_named_resource("gpus")  # a second resource: the last-ALL rule is per (worker, resource)
    shapes = [TB().cpus(1), TB().cpus(2), TB().cpus_all(), TB().cpus(0.5), TB().cpus(3).next_variant().cpus(1),
              TB().cpus(1).add_resource(gpu, 1), TB().cpus(1).add_all(gpu), TB().add_resource(gpu, 0.5)]
    for c in [int(x) for x in np.random.default_rng(seed).integers(2, 6, size=4)]:
        e.new_worker(WB(c).res_sum("gpus", 2))
    prio, n_msgs, removed, uploaded, n_ticks = 0, 0, 0, False, 0
    try:
        for round_ in range(8):
            for _ in range(int(rng.integers(1, 7)) if round_ else int(rng.integers(8, 16))):
                e.new_task(shapes[int(rng.integers(0, len(shapes)))].user_priority(prio))
            if rng.random() < 0.6:
                prio += 1
            new_msgs = e.retract_messages[n_msgs:]; n_msgs = len(e.retract_messages)
            if new_msgs and uploaded:
                a.retracting_add([t for (_, t) in new_msgs], [w for (w, _) in new_msgs])
            snap = e.snapshot()
            if not uploaded:
                a.cluster_upload(snap); a.assigned_enable([]); uploaded = True
                if new_msgs:
                    a.retracting_add([t for (_, t) in new_msgs], [w for (w, _) in new_msgs])
            try:
                # (the resident worker set emulates worker_map_rank, include/hqtick.h; no scenario here loses a worker at a size where the map's history shows, so B ticks on a map of the ids present)
                want = b.tick(dataclasses.replace(snap, worker_map_rank=None, _keep=[]))
            except HqTickError as err:
                assert err.code == abi.HQTICK_E_UNSUPPORTED
                break
            got = _ledger_tick(a, snap)
            _same(got, want)
            e.apply(want)
            n_ticks += 1
            _check_state(e, a)
            # prefilled tasks that start (task_from_prefilled_to_started, worker.rs:212-221): insert + free.remove outside a tick
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state == PREFILLED and rng.random() < 0.3:
                    _start_prefilled(e, t.id)
                    assert a.assigned_add([(t.id, t.worker, t.rq, 0, t.priority)]) == 1 and a.assigned_last_unknown() == 0
            _check_state(e, a)
            # finishes and rejects of running tasks: one release batch, in the order SchedEnv applies them
            batch = []
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state in (ASSIGNED, RUNNING) and rng.random() < 0.35:
                    if t.state == ASSIGNED and rng.random() < 0.25:
                        wid, v = t.worker, t.rv
                        e.reject_task(t.id, wid, v)
                        a.cluster_set_blocked(wid, sorted(e.workers[wid].blocked_requests))
                    else:
                        e.finish_task(t.id, t.worker)
                    batch.append(t.id)
            perm = batch[:]  # (the ledger applies a batch in ITS order; SchedEnv applied these ids in ascending order)
            assert a.assigned_release(perm) == len(batch) and a.assigned_last_unknown() == 0
            new_msgs = e.retract_messages[n_msgs:]; n_msgs = len(e.retract_messages)
            if new_msgs:
                a.retracting_add([t for (_, t) in new_msgs], [w for (w, _) in new_msgs])
            _check_state(e, a)
            # a worker joins
            if rng.random() < 0.3:
                wid = e.new_worker(WB(int(rng.integers(2, 6))))
                s2 = e.snapshot(); i = s2.worker_id.tolist().index(wid)
                tot = np.asarray(s2.worker_total, np.uint64).reshape(len(s2.worker_id), s2.n_resources)[i:i + 1]
                a.cluster_add_workers([wid], tot, tot)
                _check_state(e, a)
            # a worker is lost (never the last two)
            busy = [w for w, x in sorted(e.workers.items()) if x.assigned_tasks]
            if busy and len(e.workers) > 2 and removed < 2 and rng.random() < 0.5:
                wid = busy[int(rng.integers(0, len(busy)))]
                if any(e.tasks[x].state == RETRACTING and x not in e.redirects for x in e.workers[wid].assigned_tasks):
                    continue  # the reference asserts in on_remove_worker (reactor.rs:90): not a scenario
                if e.workers[wid].prefilled_tasks:
                    continue  # (SchedEnv.remove_worker cannot dissolve a prefill set of the worker it has just dropped; prefills are not the ledger's)
                back = sorted(e.workers[wid].assigned_tasks)
                sent = e.remove_worker(wid)
                assert a.cluster_remove_workers([wid]) == sent
                assert a.cluster_last_requeued() == [(t, e.tasks[t].rq, e.tasks[t].priority) for t in back]
                removed += 1
                new_msgs = e.retract_messages[n_msgs:]; n_msgs = len(e.retract_messages)
                if new_msgs:
                    a.retracting_add([t for (_, t) in new_msgs], [w for (w, _) in new_msgs])
                _check_state(e, a)
            assert a.retracting_count() == sum(1 for t in e.tasks.values() if t.state == RETRACTING)
        assert n_ticks >= 2, n_ticks  # (a seed whose first tick is already refused would test nothing)
    finally:
        a.close(); b.close()


def _start_prefilled(e, tid):
    """SchedEnv has no task_from_prefilled_to_started: the task leaves its prefill set and runs on its worker with variant 0 (insert_sn_task)"""
    t = e.tasks[tid]
    w = e.workers[t.worker]
    w.prefilled_tasks.discard(tid)
    e.prefill[t.rq][1].remove(tid)
    t.state, t.rv = RUNNING, 0
    e._remove(w, t.rq, 0)
    w.assigned_tasks.add(tid)


def _one_worker_env():
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

    e = SchedEnv(abi.make_config(time_limit_s=20.0))
    wid = e.new_worker(WB(8))
    amt = [e.new_task_running(TB().cpus(1), wid) for _ in range(2)]
    al = e.new_task_running(TB().cpus_all(), wid)
    amt.append(e.new_task_running(TB().cpus(2), wid))
    return e, wid, amt, al


@pytest.mark.parametrize("order", ["amount_first", "all_first", "mixed"])
def test_release_batch_is_applied_in_its_order(order):
    """On one worker, ALL and AMOUNT releases in one batch: the result is SchedEnv's applied one by one in the batch's order (an order-blind sum fails)"""
    from hyperqueue_amd.tick import Tick

    e, wid, amt, al = _one_worker_env()
    seq = {"amount_first": amt + [al], "all_first": [al] + amt, "mixed": [amt[0], al, amt[1], amt[2]]}[order]
    t = Tick(abi.make_config(time_limit_s=20.0))
    try:
        snap = e.snapshot()
        t.cluster_upload(snap)
        t.assigned_enable([(x, wid, e.tasks[x].rq, e.tasks[x].rv, e.tasks[x].priority) for x in sorted(e.workers[wid].assigned_tasks)])
        assert t.assigned_count() == 4
        for x in seq:
            e.finish_task(x, wid)
        assert t.assigned_release(seq) == 4 and t.assigned_count() == 0
        want = np.asarray(e.snapshot().worker_free, np.uint64).reshape(1, -1)
        assert (t.assigned_free_rows() == want).all()
        total = int(np.asarray(snap.worker_total, np.uint64).reshape(-1)[0])
        expect = {"amount_first": total, "all_first": total + 4 * 10_000, "mixed": total + 3 * 10_000}[order]
        assert int(want[0, 0]) == expect
    finally:
        t.close()


def test_unknown_and_repeated_ids_are_counted_and_change_nothing():
    from hyperqueue_amd.tick import Tick

    e, wid, amt, al = _one_worker_env()
    t = Tick(abi.make_config(time_limit_s=20.0))
    try:
        t.cluster_upload(e.snapshot())
        t.assigned_enable([(x, wid, e.tasks[x].rq, e.tasks[x].rv, e.tasks[x].priority) for x in sorted(e.workers[wid].assigned_tasks)])
        before = t.assigned_free_rows()
        assert t.assigned_release([10 ** 12, 10 ** 12 + 1]) == 0 and t.assigned_last_unknown() == 2
        assert (t.assigned_free_rows() == before).all() and t.assigned_count() == 4
        e.finish_task(amt[0], wid)
        assert t.assigned_release([amt[0], amt[0], 10 ** 12]) == 1 and t.assigned_last_unknown() == 2
        assert (t.assigned_free_rows() == np.asarray(e.snapshot().worker_free, np.uint64).reshape(1, -1)).all()
        # an id already in the ledger is not entered twice
        x = amt[1]
        assert t.assigned_add([(x, wid, e.tasks[x].rq, 0, e.tasks[x].priority)]) == 0 and t.assigned_last_unknown() == 1
        assert t.assigned_count() == 3
        # a task that starts outside a tick: insert + free.remove
        from hyperqueue_amd.core import TaskBuilder as TB
        y = e.new_task(TB().cpus(1))
        e.assign_and_start_task(y, wid, 0)
        assert t.assigned_add([(y, wid, e.tasks[y].rq, 0, e.tasks[y].priority)]) == 1
        assert (t.assigned_free_rows() == np.asarray(e.snapshot().worker_free, np.uint64).reshape(1, -1)).all()
        w, v = t.assigned_lookup([y, amt[0]])
        assert w.tolist() == [wid, abi.HQ_NO_WORKER] and v.tolist() == [0, 0xFF]
    finally:
        t.close()


def test_errors():
    from hyperqueue_amd import workloads
    from hyperqueue_amd.tick import HqTickError, Tick

    snap = workloads.make_steady("c3", seed=5, n_tasks=4_000, n_workers=8)
    t = Tick(abi.make_config(time_limit_s=20.0))
    try:
        with pytest.raises(HqTickError) as err:
            t.assigned_enable([])
        assert err.value.code == abi.HQTICK_E_INVALID  # no resident worker set
        t.cluster_upload(snap)
        t.assigned_enable([])
        with pytest.raises(HqTickError) as err:
            t.tick(snap, resident_workers=True)  # the snapshot still carries its assigned CSR: two truths
        assert err.value.code == abi.HQTICK_E_INVALID
        t._lib.hqtick_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        assert t._lib.hqtick_set_shard(t._ctx, 0, 2) == abi.HQTICK_E_UNSUPPORTED
        t.assigned_disable()
        assert t._lib.hqtick_set_shard(t._ctx, 0, 2) == 0
        with pytest.raises(HqTickError) as err:
            t.assigned_enable([])
        assert err.value.code == abi.HQTICK_E_UNSUPPORTED
    finally:
        t.close()


def _resident_pair(flags_a, flags_b, env_b=None, n_tasks=60_000, n_workers=64, seed=7, name="c3"):
    import os

    from hyperqueue_amd import workloads
    from hyperqueue_amd.tick import Tick

    snap = workloads.make_steady(name, seed=seed, n_tasks=n_tasks, n_workers=n_workers)
    snap = dataclasses.replace(snap, assigned=[[] for _ in snap.worker_id], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    out = []
    for flags, env in ((flags_a, None), (flags_b, env_b)):
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            t = Tick(abi.make_config(time_limit_s=20.0, flags=flags))
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        t.cluster_upload(snap)
        t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        t.assigned_enable([])
        out.append(t)
    return snap, out


def _resident_tick(t, snap):
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    return abi.parse_result(t.tick_raw(sc, resident=True), len(snap.worker_id), snap.n_resources)


def test_two_call_and_consume_in_tick_feed_the_same_ledger():
    from hyperqueue_amd.tick import HqTickError

    snap, (x, y) = _resident_pair(0, abi.HQTICK_FLAG_CONSUME_IN_TICK)
    try:
        for _ in range(3):
            before = x.assigned_count()
            rx = _resident_tick(x, snap)
            with pytest.raises(HqTickError) as err:
                x.assigned_release([1])  # the placement is pending until consumed
            assert err.value.code == abi.HQTICK_E_INVALID
            x.ready_consume_last()
            ry = _resident_tick(y, snap)
            assert rx.records == ry.records and (rx.new_free == ry.new_free).all()
            n_asg = sum(1 for w in rx.records for r in w if r[2] == abi.HQ_REC_ASSIGN)
            assert n_asg > 0 and x.assigned_count() == y.assigned_count() == before + n_asg
            assert (x.assigned_free_rows() == y.assigned_free_rows()).all() and (x.assigned_free_rows() == rx.new_free).all()
            ids = sorted(r[0] for w in rx.records for r in w)
            assert [a.tolist() for a in x.assigned_lookup(ids)] == [a.tolist() for a in y.assigned_lookup(ids)]
            # release half of what runs, in the same order on both
            run = [r[0] for w in rx.records for r in w if r[2] == abi.HQ_REC_ASSIGN][::2]
            assert x.assigned_release(run) == y.assigned_release(run) == len(run)
            assert (x.assigned_free_rows() == y.assigned_free_rows()).all()
    finally:
        x.close(); y.close()


def test_ordered_view_feeds_the_same_ledger():
    snap, (x, y) = _resident_pair(abi.HQTICK_FLAG_CONSUME_IN_TICK, abi.HQTICK_FLAG_CONSUME_IN_TICK, env_b={"HQTICK_ORDERED_VIEW": "1"})
    try:
        for _ in range(2):
            rx, ry = _resident_tick(x, snap), _resident_tick(y, snap)
            assert rx.records == ry.records
            assert x.assigned_count() == y.assigned_count() > 0
            assert (x.assigned_free_rows() == y.assigned_free_rows()).all()
            ids = sorted(r[0] for w in rx.records for r in w)
            assert [a.tolist() for a in x.assigned_lookup(ids)] == [a.tolist() for a in y.assigned_lookup(ids)]
    finally:
        x.close(); y.close()


def test_resident_loop_at_c3p_scale_matches_the_row_delta_protocol():
    """1 M tasks, 1024 workers: add -> tick -> release of the previous step's tasks.  A keeps the ledger; B sends the free rows of every change and the
    assigned CSR, as today.  Every tick equal, the ledger's count = the running tasks."""
    from hyperqueue_amd import workloads
    from hyperqueue_amd.tick import Tick

    snap = workloads.make_steady("c3p", seed=3, n_tasks=1_000_000, n_workers=1024)
    W, R = len(snap.worker_id), snap.n_resources
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    cfg = abi.make_config(time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK)
    a, b = Tick(cfg), Tick(cfg)
    try:
        for t in (a, b):
            t.cluster_upload(snap); t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        a.assigned_enable([])
        running = {}  # task -> (worker index, rq, variant)
        total = np.asarray(snap.worker_total, np.uint64).reshape(W, R)
        free = total.copy()
        rq_of = dict(zip(snap.task_id.tolist(), snap.task_rq.tolist()))
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
            ra = _resident_tick(a, snap)
            sc = sb.to_c(resident_workers=True)
            rb = abi.parse_result(b.tick_raw(sc, resident=True), W, R)
            assert ra.records == rb.records and ra.counts == rb.counts and (ra.new_free == rb.new_free).all()
            nf = np.asarray(rb.new_free, np.uint64).reshape(W, R)
            changed = np.nonzero((nf != free).any(axis=1))[0].tolist()  # today's protocol: the rows the tick itself changed go back as deltas
            free = nf.copy()
            if changed:
                b.cluster_update_workers(changed, free[changed])
            new = []
            for w, recs in enumerate(rb.records):
                for (tid, v, kind) in recs:
                    if kind == abi.HQ_REC_ASSIGN:
                        running[tid] = (w, rq_of[tid], v); new.append(tid)
            assert a.assigned_count() == len(running)
            # the previous step's tasks finish: A releases them, B sends the rows they touched (computed as the reference does, one by one)
            if prev:
                assert a.assigned_release(prev) == len(prev)
                touched = set()
                ent = _entries(snap)
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


def _entries(snap):
    """rq -> variant -> [(resource, kind, amount)]"""
    return [[[(int(r), int(k), int(a)) for (r, k, a) in v["entries"]] for v in rq] for rq in snap.requests]


def _pair_no_ledger_b(n_tasks=40_000, n_workers=32, seed=9):
    from hyperqueue_amd import workloads
    from hyperqueue_amd.tick import Tick

    snap = workloads.make_steady("c3", seed=seed, n_tasks=n_tasks, n_workers=n_workers)
    snap = dataclasses.replace(snap, assigned=[[] for _ in snap.worker_id], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    a, b = Tick(abi.make_config(time_limit_s=20.0)), Tick(abi.make_config(time_limit_s=20.0))
    for t in (a, b):
        t.cluster_upload(snap); t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    a.assigned_enable([])
    return snap, a, b


def test_an_abandoned_two_call_tick_never_enters_the_ledger():
    """two-call tick, then a ready-set delta that drops its selection (the append path of hqtick_ready_add_packed), then consume: the tick's tasks stay
    in the ready set, so the ledger and the free rows must not take them"""
    snap, a, b = _pair_no_ledger_b()
    try:
        free0 = a.assigned_free_rows()
        r = _resident_tick(a, snap)
        assert sum(len(w) for w in r.records) > 0
        top = int(snap.task_id.max()) + 1
        a.ready_add_packed([(top, 16)], [(0, 16)], np.zeros(16, np.uint16))
        live = a.ready_count()
        a.ready_consume_last()
        assert a.ready_count() == live and a.assigned_count() == 0
        assert (a.assigned_free_rows() == free0).all()
        assert a.assigned_release([top]) == 0 and a.assigned_last_unknown() == 1  # nothing pending any more: the ledger takes calls
        # the next tick places again, and this time its placement enters
        r2 = _resident_tick(a, snap)
        a.ready_consume_last()
        n_asg = sum(1 for w in r2.records for x in w if x[2] == abi.HQ_REC_ASSIGN)
        assert n_asg > 0 and a.assigned_count() == n_asg and (a.assigned_free_rows() == r2.new_free).all()
    finally:
        a.close(); b.close()


def test_a_lost_workers_tasks_go_back_into_the_resident_ready_set():
    """resident ready set + ledger (A) against the resident ready set with the host's bookkeeping (B): a busy worker is lost; A puts its tasks back into the
    ready set on its own (hqtick_cluster_last_requeued), B re-adds them with hqtick_ready_add; the ready sets and the next ticks are the same"""
    snap, a, b = _pair_no_ledger_b()
    try:
        W, R = len(snap.worker_id), snap.n_resources
        meta = {int(t): (int(q), int(p)) for t, q, p in zip(snap.task_id, snap.task_rq, snap.task_priority)}
        ra = _resident_tick(a, snap)
        rb = abi.parse_result(b.tick_raw(snap.to_c(resident_workers=True), resident=True), W, R)
        assert ra.records == rb.records and (ra.new_free == rb.new_free).all()
        a.ready_consume_last(); b.ready_consume_last()
        free = np.asarray(rb.new_free, np.uint64).reshape(W, R)
        b.cluster_update_workers(list(range(W)), free)
        running = [[(tid, v) for (tid, v, k) in rb.records[w] if k == abi.HQ_REC_ASSIGN] for w in range(W)]
        wi = max(range(W), key=lambda w: len(running[w]))
        wid = int(snap.worker_id[wi])
        assert running[wi]
        back = sorted(tid for tid, _ in running[wi])
        assert a.cluster_remove_workers([wid]) == [] and b.cluster_remove_workers([wid]) == []
        want = [(t, meta[t][0], meta[t][1]) for t in back]
        assert a.cluster_last_requeued() == want
        b.ready_add([t for t, _, _ in want], [p for _, _, p in want], [q for _, q, _ in want])
        assert a.ready_count() == b.ready_count()
        keep = [w for w in range(W) if w != wi]
        per_w = [[(meta[tid][0], v) for tid, v in running[w]] for w in keep]
        s2 = dataclasses.replace(snap, worker_id=snap.worker_id[keep], worker_total=np.asarray(snap.worker_total, np.uint64).reshape(W, R)[keep].reshape(-1),
                                 worker_free=free[keep].reshape(-1), worker_remaining_ns=snap.worker_remaining_ns[keep], worker_min_utilization=snap.worker_min_utilization[keep],
                                 worker_flags=snap.worker_flags[keep], worker_group=snap.worker_group[keep], assigned=per_w, prefilled=[[] for _ in keep], blocked=[], _keep=[])
        assert (a.assigned_free_rows() == free[keep]).all()
        ra2 = _resident_tick(a, s2)
        rb2 = abi.parse_result(b.tick_raw(s2.to_c(resident_workers=True), resident=True), len(keep), R)
        assert ra2.records == rb2.records and ra2.counts == rb2.counts and (ra2.new_free == rb2.new_free).all()
        assert a.ready_remove(back) == b.ready_remove(back) == len(back)  # the requeued tasks are in the resident ready set (the tick left them there)
    finally:
        a.close(); b.close()
