"""The growth paths of the assignment ledger that the random scenarios of test_gpu_assigned*.py never reach: they use at most nine variant
slots and a few dozen entries, so the hash table is never rebuilt and no row table is ever widened outside the 1 M-task loops.  Here: a rebuild of the hash
table with tombstones in it (twice, so that the columns swapped out by the first rebuild are the target of the second), count rows widened from 16 to 32
slots, prefilled rows widened from 16 to 32 requests, a membership change while both are wide, and a second hqtick_assigned_enable on a ledger that holds
entries, multi-node rows and prefilled tracking.  Expected state is SchedEnv's (hyperqueue_amd/core.py), expected ticks are those of a second context on
SchedEnv's full snapshot — never the ledger's own answers."""
import dataclasses

import numpy as np
import pytest

from hyperqueue_amd import abi

pytestmark = pytest.mark.gpu

WAITING, ASSIGNED, RUNNING, PREFILLED, RETRACTING, RUNNING_MN = 0, 1, 2, 3, 4, 5
PF = 0xFE


def _same(a, b):
    assert a.status == b.status and a.is_optimal == b.is_optimal and a.batches == b.batches
    assert a.counts == b.counts and a.records == b.records and a.retracts == b.retracts
    assert (a.new_free == b.new_free).all()
    assert a.redirects == b.redirects and a.redirect_kinds == b.redirect_kinds
    assert a.mn == b.mn


def _ledger_tick(t, snap, tracking):
    """a tick of the ledger context: resident workers, resident Retracting table, no assigned CSR and (tracking on) no prefilled CSR"""
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    if tracking:
        sc.prefilled_off = None; sc.prefilled_rq = None
    sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None
    sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
    return abi.parse_result(t.tick_raw(sc), len(snap.worker_id), snap.n_resources)


def _b_tick(b, snap):
    return b.tick(dataclasses.replace(snap, worker_map_rank=None, _keep=[]))


def _check_state(e, t, flags=False):
    """free rows, every id ever used (assigned with its variant, prefilled, multi-node, absent) and the three counts against SchedEnv"""
    snap = e.snapshot()
    W = len(snap.worker_id)
    assert t.cluster_workers().tolist() == sorted(e.workers)
    assert (t.assigned_free_rows() == np.asarray(snap.worker_free, np.uint64).reshape(W, snap.n_resources)).all()
    if flags:
        assert t.cluster_worker_flags().tolist() == np.asarray(snap.worker_flags).tolist()
    mn = {x.id: x.mn_workers for x in e.tasks.values() if x.state == RUNNING_MN}
    ids = sorted(e.tasks)
    w, v = t.assigned_lookup(ids)
    got_a, got_p = {}, {}
    for tid, wid, var in zip(ids, w.tolist(), v.tolist()):
        if tid in mn:
            assert (wid, var) == (mn[tid][0], 0xFF)  # a multi-node id answers with its root
        elif wid == abi.HQ_NO_WORKER:
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
    assert t.assigned_mn_count() == len(mn)
    for tid, ws in mn.items():
        assert t.assigned_mn_workers(tid) == [ws[0]] + sorted(ws[1:]), tid


def _entry(e, tid):
    x = e.tasks[tid]
    return (tid, x.worker, x.rq, x.rv, x.priority)


# ---------------------------------------------------------------------------------------------- 1: the hash table is rebuilt with tombstones in it
def test_table_rebuild_with_tombstones():
    """The table is rebuilt when (live + tombstones + batch) x 2 exceeds its buckets, into 1024 buckets or the first power of two >= (live + batch) x 4.
    256 entries are the most a first table of 1024 buckets takes (256 x 4 = 1024).  Cycle 1: release 206 (50 live, 206 tombstones), add 260 ->
    (50 + 206 + 260) x 2 = 1032 > 1024: a rebuild into 2048 buckets.  Cycle 2: release 260 (50 live, 260 tombstones), add 720 -> 1030 x 2 = 2060 > 2048: a
    rebuild into 4096 buckets whose target columns are the ones cycle 1 swapped out."""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import Tick

    cfg = abi.make_config(time_limit_s=20.0)
    e = SchedEnv(cfg)
    gpu = e.new_named_resource("gpus")
    wids = e.new_workers(4, WB(1000).res_sum("gpus", 1000))
    shapes = [TB().cpus(1), TB().cpus(2).add_resource(gpu, 1), TB().cpus(0.5)]
    n_new = [0]

    def running():
        n_new[0] += 1
        return e.new_task_running(shapes[n_new[0] % 3], wids[(n_new[0] * 7) % 4])

    def start():
        n_new[0] += 1
        tid = e.new_task(shapes[n_new[0] % 3])
        e.assign_and_start_task(tid, wids[(n_new[0] * 7) % 4], 0)
        return tid

    live = [running() for _ in range(256)]
    t = Tick(cfg)
    try:
        t.cluster_upload(e.snapshot())
        t.assigned_enable([_entry(e, x) for x in live])
        _check_state(e, t)
        for n_release, n_add in ((206, 260), (260, 720)):
            gone = live[1::2][:n_release // 2] + live[::2][:n_release - n_release // 2]  # (not in id order: a release batch is applied in ITS order)
            assert len(set(gone)) == n_release
            for x in gone:
                e.finish_task(x, e.tasks[x].worker)
            assert t.assigned_release(gone) == n_release and t.assigned_last_unknown() == 0
            live = [x for x in live if x not in set(gone)]
            assert len(live) == 50
            _check_state(e, t)
            fresh = [start() for _ in range(n_add)]
            assert t.assigned_add([_entry(e, x) for x in fresh]) == n_add and t.assigned_last_unknown() == 0
            live += fresh
            _check_state(e, t)  # every id ever used: the released ones are absent, the 50 that lived through the rebuild are where they were
        assert t.assigned_count() == 770
        assert t.assigned_release(live[:50]) == 50  # an entry that has moved twice is still released with its own request
        for x in live[:50]:
            e.finish_task(x, e.tasks[x].worker)
        _check_state(e, t)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------- 2: the count rows widen from 16 to 32 variant slots
def _two_variant_shapes(gpu, n):
    from hyperqueue_amd.core import TaskBuilder as TB

    return [TB().cpus(2 + 0.25 * i).next_variant().cpus(1).add_resource(gpu, 0.25 * (i + 1)) for i in range(n)]


def test_wider_count_rows():
    """4 requests of 2 variants (8 slots: rows of 16), then 9 such requests (18 slots: rows of 32) while tasks of the first snapshot still run"""
    from hyperqueue_amd.core import SchedEnv, WorkerBuilder as WB
    from hyperqueue_amd.tick import Tick

    cfg = abi.make_config(reserve=0, fill_max=0, time_limit_s=20.0)
    e = SchedEnv(cfg)
    gpu = e.new_named_resource("gpus")
    e.new_workers(6, WB(8).res_sum("gpus", 4))
    shapes = _two_variant_shapes(gpu, 9)
    a, b = Tick(cfg), Tick(cfg)
    try:
        for s in shapes[:4]:
            e.new_tasks(3, s)
        snap = e.snapshot()
        assert len(snap.requests) == 4 and sum(len(r) for r in snap.requests) == 8
        a.cluster_upload(snap); a.assigned_enable([])
        want = _b_tick(b, snap)
        _same(_ledger_tick(a, snap, False), want)
        e.apply(want)
        first = sorted(x.id for x in e.tasks.values() if x.state == ASSIGNED)
        assert len(first) >= 8
        _check_state(e, a)
        done = first[::3]
        for x in done:
            e.finish_task(x, e.tasks[x].worker)
        assert a.assigned_release(done) == len(done)
        for s in shapes:
            e.new_tasks(2, s)
        snap = e.snapshot()
        assert len(snap.requests) == 9 and sum(len(r) for r in snap.requests) == 18
        want = _b_tick(b, snap)
        _same(_ledger_tick(a, snap, False), want)  # the rows widen under this tick
        e.apply(want)
        assert any(e.tasks[x].state == ASSIGNED for x in first) and any(x.state == ASSIGNED and x.rq >= 8 for x in e.tasks.values())
        _check_state(e, a)
        # the tasks of the first snapshot finish on rows that have moved; the next tick is the plain context's
        done = [x for x in first if e.tasks[x].state == ASSIGNED]
        for x in done:
            e.finish_task(x, e.tasks[x].worker)
        assert a.assigned_release(done) == len(done) and a.assigned_last_unknown() == 0
        _check_state(e, a)
        e.new_tasks(2, shapes[8]); e.new_tasks(2, shapes[0])
        snap = e.snapshot()
        want = _b_tick(b, snap)
        assert sum(len(w) for w in want.records) > 0
        _same(_ledger_tick(a, snap, False), want)
        e.apply(want)
        _check_state(e, a)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 3, 4: the prefilled rows widen from 16 to 32 requests
def _wide_prefilled(membership):
    """4 workers of 4 cpus, 24 one-cpu tasks, at most 2 prefilled tasks per worker: tick 1 (4 requests) assigns 16 and prefills 8; tick 2 runs on 17 requests,
    so the prefilled rows (and, 17 variant slots, the count rows) widen while the 8 prefilled tasks live.  membership: then a worker joins and one that holds
    running and prefilled tasks is lost."""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import Tick

    cfg = abi.make_config(reserve=0, fill_max=2, time_limit_s=20.0)
    e = SchedEnv(cfg)
    gpu = e.new_named_resource("gpus")
    e.new_workers(4, WB(4).res_sum("gpus", 2))
    one = TB().cpus(1)
    others = [TB().cpus(1).add_resource(gpu, 0.125 * (i + 1)) for i in range(16)]
    a, b = Tick(cfg), Tick(cfg)
    try:
        e.new_tasks(24, one)
        for s in others[:3]:
            e.rq_id(s)
        snap = e.snapshot()
        assert len(snap.requests) == 4
        a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
        want = _b_tick(b, snap)
        _same(_ledger_tick(a, snap, True), want)
        e.apply(want)
        old_pf = sorted(x.id for x in e.tasks.values() if x.state == PREFILLED)
        assert len(old_pf) == 8 and a.assigned_prefilled_count() == 8
        _check_state(e, a)
        # one assigned task of every worker finishes; tasks of the first request and of the seventeenth arrive
        done = [min(w.assigned_tasks) for _, w in sorted(e.workers.items())]
        for x in done:
            e.finish_task(x, e.tasks[x].worker)
        assert a.assigned_release(done) == len(done)
        for s in others[3:]:
            e.rq_id(s)
        e.new_tasks(8, one); e.new_tasks(2, others[15])
        snap = e.snapshot()
        assert len(snap.requests) == 17
        want = _b_tick(b, snap)  # (B is given the prefilled CSR)
        _same(_ledger_tick(a, snap, True), want)  # the rows widen under this tick
        e.apply(want)
        assert all(e.tasks[x].state == PREFILLED for x in old_pf)
        assert a.assigned_prefilled_count() == sum(len(w.prefilled_tasks) for w in e.workers.values()) >= 8
        _check_state(e, a)
        e.start_prefilled_task(old_pf[0], 0)
        assert a.assigned_start_prefilled([(old_pf[0], 0)]) == 1 and a.assigned_last_unknown() == 0
        e.cancel_prefilled_task(old_pf[1])
        assert a.assigned_unprefill([old_pf[1]]) == 1 and a.assigned_last_unknown() == 0
        _check_state(e, a)
        if membership:
            wid = e.new_worker(WB(4).res_sum("gpus", 2))
            s2 = e.snapshot(); i = s2.worker_id.tolist().index(wid)
            tot = np.asarray(s2.worker_total, np.uint64).reshape(len(s2.worker_id), s2.n_resources)[i:i + 1]
            a.cluster_add_workers([wid], tot, tot)
            _check_state(e, a)
            lost = next(w for w, x in sorted(e.workers.items()) if x.assigned_tasks and x.prefilled_tasks)
            x = e.workers[lost]
            snap = e.snapshot()
            a.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)  # the requeued tasks go back into a resident ready set
            pf_back = sorted(x.prefilled_tasks)
            back = [(t, e.tasks[t].rq, e.tasks[t].priority) for t in sorted(set(x.assigned_tasks) | set(x.prefilled_tasks))]
            assert pf_back and len(back) > len(pf_back)
            sent = e.remove_worker(lost)
            assert a.cluster_remove_workers([lost]) == sent
            assert a.cluster_last_requeued() == back
            assert a.cluster_last_requeued_prefilled() == pf_back
            assert a.ready_count() == len(e.snapshot().task_id)
            _check_state(e, a)
        # the next tick: two more tasks finish, tasks of the first and the seventeenth request arrive
        done = sorted(x.id for x in e.tasks.values() if x.state in (ASSIGNED, RUNNING))[:2]
        for x in done:
            e.finish_task(x, e.tasks[x].worker)
        assert a.assigned_release(done) == len(done)
        e.new_tasks(4, one); e.new_tasks(2, others[15])
        snap = e.snapshot()
        want = _b_tick(b, snap)
        assert sum(len(w) for w in want.records) + len(want.redirects) > 0
        _same(_ledger_tick(a, snap, True), want)
        e.apply(want)
        _check_state(e, a)
    finally:
        a.close(); b.close()


def test_wider_prefilled_rows():
    _wide_prefilled(membership=False)


def test_membership_change_while_both_tables_are_wide():
    _wide_prefilled(membership=True)


# ---------------------------------------------------------------------------------------------- 5: hqtick_assigned_enable on a ledger that holds everything
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


def test_enable_twice():
    """The second list names other tasks of the same shapes on the same workers (the free rows are the resident ones and stay as they are): the ledger answers
    for the second list alone, holds no prefilled entry and no multi-node row, and tracking is off until it is asked for again"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import HqTickError, Tick

    cfg = abi.make_config(fill_max=2, time_limit_s=20.0)
    e = SchedEnv(cfg)
    gpu = e.new_named_resource("gpus")
    wids = e.new_workers(6, WB(8).res_sum("gpus", 2))
    shapes = [TB().cpus(1), TB().cpus(2).add_resource(gpu, 1), TB().cpus(3).next_variant().cpus(1)]
    run1 = [e.new_task_running(shapes[i % 3], wids[i % 2]) for i in range(6)]
    mn = e.new_task(TB().n_nodes(2).user_priority(1))
    pf1 = [_make_prefilled(e, TB().cpus(1), wids[2]), _make_prefilled(e, TB().cpus(1), wids[2]), _make_prefilled(e, shapes[1], wids[3])]
    t = Tick(cfg)
    try:
        t.cluster_upload(e.snapshot())
        t.assigned_enable([_entry(e, x) for x in run1])
        assert t.assigned_add_mn([(mn, e.tasks[mn].rq, e.tasks[mn].priority, [wids[4], wids[5]])]) == 1 and t.assigned_last_unknown() == 0
        e.start_task_mn(mn, [wids[4], wids[5]])
        seed = [(x, e.tasks[x].worker, e.tasks[x].rq, e.tasks[x].priority) for x in pf1]
        assert t.assigned_track_prefilled(seed) == 3 and t.assigned_last_unknown() == 0
        assert (t.assigned_count(), t.assigned_mn_count(), t.assigned_prefilled_count()) == (6, 1, 3)
        _check_state(e, t, flags=True)
        # what the second list describes: every running task replaced by a new one of its shape on its worker, the prefilled tasks cancelled
        run2 = []
        for x in run1:
            wid, rq = e.tasks[x].worker, e.tasks[x].rq
            e.finish_task(x, wid)
            y = e.new_task(shapes[run1.index(x) % 3])
            assert e.tasks[y].rq == rq
            e.assign_and_start_task(y, wid, 0)
            run2.append(y)
        for x in pf1:
            e.cancel_prefilled_task(x)
        t.assigned_enable([_entry(e, x) for x in run2])
        assert (t.assigned_count(), t.assigned_mn_count(), t.assigned_prefilled_count()) == (6, 0, 0)
        w, v = t.assigned_lookup(run1 + pf1 + [mn] + run2)
        assert w.tolist() == [abi.HQ_NO_WORKER] * 10 + [e.tasks[x].worker for x in run2]
        assert v.tolist() == [0xFF] * 10 + [0] * 6
        for call in (lambda: t.assigned_start_prefilled([(pf1[0], 0)]), lambda: t.assigned_unprefill([pf1[0]])):  # tracking is off
            with pytest.raises(HqTickError) as err:
                call()
            assert err.value.code == abi.HQTICK_E_INVALID
        # the host completes the new ledger: the multi-node task on its two workers (uploaded flags: the mirror's, without their SN bit), tracking with a new seed
        assert t.assigned_add_mn([(mn, e.tasks[mn].rq, e.tasks[mn].priority, [wids[4], wids[5]])]) == 1 and t.assigned_last_unknown() == 0
        pf2 = _make_prefilled(e, TB().cpus(1), wids[3])
        assert t.assigned_track_prefilled([(pf2, wids[3], e.tasks[pf2].rq, e.tasks[pf2].priority)]) == 1 and t.assigned_last_unknown() == 0
        _check_state(e, t, flags=True)
    finally:
        t.close()
