"""Multi-node tasks and worker flags on the resident worker set (hqtick_assigned_add_mn / _mn_count / _mn_workers, hqtick_cluster_set_flags /
_worker_flags).  As in test_gpu_assigned.py, context A keeps the ledger and context B runs today's protocol on SchedEnv's full snapshot
(worker_map_rank=None): every tick of A equals B's, and after every event A's free rows, flags, single-node tasks and multi-node tasks equal SchedEnv's."""
import dataclasses

import numpy as np
import pytest

from hyperqueue_amd import abi

pytestmark = pytest.mark.gpu

ASSIGNED, RUNNING, RUNNING_MN = 1, 2, 5
SN, STOPPING = abi.HQ_WORKER_SN, abi.HQ_WORKER_STOPPING
KINDS = ("root", "nonroot", "free", "busy")


def _same(a, b):
    assert a.status == b.status and a.is_optimal == b.is_optimal and a.batches == b.batches
    assert a.counts == b.counts and a.records == b.records and a.retracts == b.retracts
    assert (a.new_free == b.new_free).all()
    assert a.redirects == b.redirects and a.redirect_kinds == b.redirect_kinds
    assert a.mn == b.mn


def _strip(sc):
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    return sc


def _ledger_tick(t, snap):
    """a tick of the ledger context: resident workers, resident Retracting table, NO assigned CSR"""
    sc = _strip(snap.to_c(resident_workers=True))
    sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None
    sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
    return abi.parse_result(t.tick_raw(sc), len(snap.worker_id), snap.n_resources)


def _b_tick(b, snap):
    return b.tick(dataclasses.replace(snap, worker_map_rank=None, _keep=[]))


def _reset_free(e, wids):
    """reset_mn_task (worker.rs:172-175) sets free = total; SchedEnv does not restate it"""
    for wid in wids:
        if wid in e.workers:
            e.workers[wid].free = list(e.workers[wid].total)


def _finish_mn(e, tid):
    ws = list(e.tasks[tid].mn_workers)
    e.finish_task(tid, ws[0])
    _reset_free(e, ws)


def _kind_of(e, wid):
    w = e.workers[wid]
    if w.mn_task is not None:
        return "root" if e.tasks[w.mn_task[0]].mn_workers[0] == wid else "nonroot"
    return "busy" if w.assigned_tasks else "free"


def _lose(e, wid):
    """SchedEnv.remove_worker + the free = total of the other nodes of a lost root -> the tasks that go back to their queues, ascending"""
    w = e.workers[wid]
    if w.mn_task is None:
        back = sorted(w.assigned_tasks)
        others = []
    else:
        t = e.tasks[w.mn_task[0]]
        root = t.mn_workers[0] == wid
        back = [t.id] if root else []
        others = [x for x in t.mn_workers if x != wid] if root else []
    sent = e.remove_worker(wid)
    _reset_free(e, others)
    return back, sent


def _check_state(e, t):
    snap = e.snapshot()
    W = len(snap.worker_id)
    assert t.cluster_workers().tolist() == sorted(e.workers)
    assert (t.assigned_free_rows() == np.asarray(snap.worker_free, np.uint64).reshape(W, snap.n_resources)).all()
    assert t.cluster_worker_flags().tolist() == np.asarray(snap.worker_flags).tolist()
    mn = {x.id: x.mn_workers for x in e.tasks.values() if x.state == RUNNING_MN}
    ids = sorted(e.tasks)
    w, v = t.assigned_lookup(ids)
    got = {}
    for tid, wid, var in zip(ids, w.tolist(), v.tolist()):
        if tid in mn:
            assert (wid, var) == (mn[tid][0], 0xFF)  # a multi-node id answers with its root
        elif wid != abi.HQ_NO_WORKER:
            got.setdefault(wid, set()).add(tid)
    want = {wid: set(x.assigned_tasks) for wid, x in e.workers.items() if x.assigned_tasks}
    assert got == want
    assert t.assigned_count() == sum(len(x) for x in want.values())
    assert t.assigned_mn_count() == len(mn)
    for tid, ws in mn.items():
        assert t.assigned_mn_workers(tid) == [ws[0]] + sorted(ws[1:]), tid
    for tid in ids:
        if tid not in mn:
            assert t.assigned_mn_workers(tid) == []
            break


# ---------------------------------------------------------------------------------------------- 1: fails on the parent with the calls of ABI 12 alone
def test_the_next_tick_keeps_off_the_workers_of_a_multi_node_task():
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB
    from hyperqueue_amd.tick import Tick

    cfg = abi.make_config(fill_max=0, time_limit_s=20.0)
    e = SchedEnv(cfg)
    a, b = Tick(cfg), Tick(cfg)
    try:
        e.new_workers_cpus([5] * 5)
        mn = [e.new_task(TB().n_nodes(2).user_priority(3)) for _ in range(2)]
        for _ in range(3):
            e.new_task(TB().cpus(1))
        snap = e.snapshot()
        a.cluster_upload(snap); a.assigned_enable([])
        want = _b_tick(b, snap)
        _same(_ledger_tick(a, snap), want)
        assert sorted(t for t, _ in want.mn) == mn and sum(len(r) for r in want.records) == 3
        e.apply(want)
        for _ in range(12):
            e.new_task(TB().cpus(1))
        snap = e.snapshot()
        want = _b_tick(b, snap)
        wids = sorted(e.workers)
        assert sum(len(r) for r in want.records) == 2  # the one single-node worker has 2 of its 5 cpus left
        assert all(not want.records[i] for i, w in enumerate(wids) if e.workers[w].mn_task is not None)
        _same(_ledger_tick(a, snap), want)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 2: scenarios
N_SEEDS = 20
_LOST = {}  # seed -> kinds of the workers lost in that scenario


def _scenario(seed):
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import HqTickError, Tick

    rng = np.random.default_rng(47_000 + seed)
    cfg = abi.make_config(reserve=int(rng.integers(0, 2)), fill_max=0, time_limit_s=20.0)
    e = SchedEnv(cfg)
    b, a = Tick(cfg), Tick(cfg)
    gpu = e.new_named_resource("gpus")
    shapes = [TB().cpus(1), TB().cpus(2), TB().cpus_all(), TB().cpus(0.5), TB().cpus(3).next_variant().cpus(1),
              TB().cpus(1).add_resource(gpu, 1), TB().cpus(1).add_all(gpu), TB().add_resource(gpu, 0.5), TB().n_nodes(2), TB().n_nodes(3)]
    for c in [int(x) for x in rng.integers(2, 6, size=int(rng.integers(6, 10)))]:
        e.new_worker(WB(c).res_sum("gpus", 2))
    prio, removed, uploaded, n_ticks, kinds = 0, 0, False, 0, []
    try:
        for round_ in range(8):
            for _ in range(int(rng.integers(1, 7)) if round_ else int(rng.integers(8, 16))):
                e.new_task(shapes[int(rng.integers(0, len(shapes)))].user_priority(prio + int(rng.integers(0, 2))))
            if rng.random() < 0.6:
                prio += 1
            snap = e.snapshot()
            if not uploaded:
                a.cluster_upload(snap); a.assigned_enable([]); uploaded = True
            try:
                want = _b_tick(b, snap)
            except HqTickError as err:
                assert err.code == abi.HQTICK_E_UNSUPPORTED
                break
            _same(_ledger_tick(a, snap), want)
            e.apply(want)
            n_ticks += 1
            _check_state(e, a)
            # finishes: single- and multi-node ids in ONE release batch, in the order SchedEnv applies them
            batch = []
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state in (ASSIGNED, RUNNING) and rng.random() < 0.35:
                    e.finish_task(t.id, t.worker); batch.append(t.id)
                elif t.state == RUNNING_MN and rng.random() < 0.35:
                    _finish_mn(e, t.id); batch.append(t.id)
            assert a.assigned_release(batch[:]) == len(batch) and a.assigned_last_unknown() == 0
            _check_state(e, a)
            # a worker joins
            if rng.random() < 0.4:
                wid = e.new_worker(WB(int(rng.integers(2, 6))).res_sum("gpus", 2))
                s2 = e.snapshot(); i = s2.worker_id.tolist().index(wid)
                tot = np.asarray(s2.worker_total, np.uint64).reshape(len(s2.worker_id), s2.n_resources)[i:i + 1]
                a.cluster_add_workers([wid], tot, tot)
                _check_state(e, a)
            # a worker is lost: the kind rotates with seed and round (a root, a non-root, a free worker, a worker with single-node tasks)
            if len(e.workers) > 4 and removed < 3 and rng.random() < 0.6:
                by_kind = {}
                for wid in sorted(e.workers):
                    by_kind.setdefault(_kind_of(e, wid), []).append(wid)
                k = KINDS[(seed + round_) % len(KINDS)]
                if k not in by_kind:
                    k = sorted(by_kind)[int(rng.integers(0, len(by_kind)))]
                wid = by_kind[k][int(rng.integers(0, len(by_kind[k])))]
                back, sent = _lose(e, wid)
                assert a.cluster_remove_workers([wid]) == sent == []
                assert a.cluster_last_requeued() == [(t, e.tasks[t].rq, e.tasks[t].priority) for t in back]
                removed += 1; kinds.append(k)
                _check_state(e, a)
        assert n_ticks >= 2, n_ticks
    finally:
        a.close(); b.close()
    _LOST[seed] = kinds


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_ledger_follows_sched_env_with_multi_node_tasks(seed):
    _scenario(seed)


def test_the_scenarios_lose_roots_non_roots_and_free_workers():
    for seed in range(N_SEEDS):  # (a run that selected only this test plays the scenarios itself)
        if seed not in _LOST:
            _scenario(seed)
    seen = {k for kinds in _LOST.values() for k in kinds}
    assert {"root", "nonroot", "free"} <= seen, _LOST


# ---------------------------------------------------------------------------------------------- 3: rows across wavefront boundaries
MN_ROWS = [[0, 63, 64], [65, 129], [1, 2, 3, 127, 128]]


def _wide_env():
    """130 workers (rows = id - 50); single-node tasks incl. ALL requests on rows outside MN_ROWS; three multi-node tasks still waiting"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

    e = SchedEnv(abi.make_config(fill_max=0, time_limit_s=20.0))
    gpu = e.new_named_resource("gpus")
    wids = e.new_workers(130, WB(8).res_sum("gpus", 2))
    assert wids == list(range(50, 180))
    sn = []
    for row in (4, 10, 62, 66, 100, 126):
        w = wids[row]
        sn.append(e.new_task_running(TB().cpus(1), w))
        sn.append(e.new_task_running(TB().cpus_all(), w))
        sn.append(e.new_task_running(TB().cpus(2).add_all(gpu), w))
        sn.append(e.new_task_running(TB().cpus(1).add_resource(gpu, 1), w))
    mn = [e.new_task(TB().n_nodes(len(rows)).user_priority(i)) for i, rows in enumerate(MN_ROWS)]
    # rows 63 and 129 carry more than their total (what "ALL, then AMOUNT" in one release leaves behind): reset_mn_task must bring them back to the total
    e.workers[wids[63]].free[0] += 10_000; e.workers[wids[129]].free[0] += 20_000
    return e, wids, sn, mn


def _wide_ctx(e, wids, mn):
    from hyperqueue_amd.tick import Tick

    t = Tick(abi.make_config(fill_max=0, time_limit_s=20.0))
    t.cluster_upload(e.snapshot())
    t.assigned_enable([(x.id, x.worker, x.rq, x.rv, x.priority) for x in sorted(e.tasks.values(), key=lambda x: x.id) if x.state == RUNNING])
    entries = [(tid, e.tasks[tid].rq, e.tasks[tid].priority, [wids[r] for r in rows]) for tid, rows in zip(mn, MN_ROWS)]
    assert t.assigned_add_mn(entries) == 3 and t.assigned_last_unknown() == 0
    return t


def _start_all_mn(e, wids, mn):
    for tid, rows in zip(mn, MN_ROWS):
        e.start_task_mn(tid, [wids[r] for r in rows])


@pytest.mark.parametrize("order", ["mn_first", "mn_last", "interleaved"])
def test_a_release_batch_of_single_and_multi_node_ids_resets_only_the_listed_rows(order):
    e, wids, sn, mn = _wide_env()
    t = _wide_ctx(e, wids, mn)
    try:
        _start_all_mn(e, wids, mn)
        _check_state(e, t)
        flags = t.cluster_worker_flags()
        listed = sorted(r for rows in MN_ROWS for r in rows)
        assert [i for i in range(130) if not flags[i] & SN] == listed
        free0 = t.assigned_free_rows()
        half = sn[::2] + sn[1::4]  # both ALL tasks of some rows before and after AMOUNT tasks of the same row
        batch = {"mn_first": mn + half, "mn_last": half[::-1] + mn[::-1],
                 "interleaved": half[:5] + [mn[1]] + half[5:11] + [mn[2], mn[0]] + half[11:]}[order]
        for tid in batch:
            if tid in mn:
                _finish_mn(e, tid)
            else:
                e.finish_task(tid, e.tasks[tid].worker)
        assert t.assigned_release(batch) == len(batch) and t.assigned_last_unknown() == 0
        _check_state(e, t)  # SchedEnv applied the batch one by one in its order: the last-ALL rule of the single-node rows is intact
        free1 = t.assigned_free_rows()
        total = np.asarray(e.snapshot().worker_total, np.uint64).reshape(130, -1)
        touched = {e.tasks[x].worker - 50 for x in half}
        for row in range(130):
            if row in listed:
                assert (free1[row] == total[row]).all()
            elif row not in touched:
                assert (free1[row] == free0[row]).all()
        assert (t.cluster_worker_flags() == SN).all() and t.assigned_mn_count() == 0
    finally:
        t.close()


def test_a_root_and_a_non_root_lost_in_one_call_in_either_order():
    states = []
    for ids in ([114, 115], [115, 114]):  # rows 64 (a non-root of the first task) and 65 (the root of the second)
        e, wids, sn, mn = _wide_env()
        t = _wide_ctx(e, wids, mn)
        try:
            _start_all_mn(e, wids, mn)
            back = []
            for wid in ids:
                back += _lose(e, wid)[0]
            assert back == [mn[1]]
            assert t.cluster_remove_workers(ids) == []
            assert t.cluster_last_requeued() == [(mn[1], e.tasks[mn[1]].rq, e.tasks[mn[1]].priority)]
            _check_state(e, t)
            assert t.assigned_mn_workers(mn[0]) == [wids[0], wids[63]] and t.assigned_mn_workers(mn[1]) == []
            states.append((t.assigned_free_rows().tolist(), t.cluster_worker_flags().tolist(), t.assigned_mn_count(), t.assigned_count()))
            # row 129 (now row 127) was the lost root's other node: a free single-node worker with its total again
            assert t.cluster_worker_flags()[127] == SN and states[-1][0][127][0] == 8 * 10_000
        finally:
            t.close()
    assert states[0] == states[1]


# ---------------------------------------------------------------------------------------------- 4: refusals of hqtick_assigned_add_mn
def test_add_mn_refusals_are_counted_and_change_nothing():
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB
    from hyperqueue_amd.tick import Tick

    e = SchedEnv(abi.make_config(fill_max=0, time_limit_s=20.0))
    w = e.new_workers_cpus([4] * 6)
    busy = e.new_task_running(TB().cpus(1), w[0])
    m = [e.new_task(TB().n_nodes(2)) for _ in range(3)]
    rq_mn, rq_sn = e.tasks[m[0]].rq, e.tasks[busy].rq
    e.workers[w[1]].stopping = True
    t = Tick(abi.make_config(fill_max=0, time_limit_s=20.0))
    try:
        t.cluster_upload(e.snapshot())
        t.assigned_enable([(busy, w[0], rq_sn, 0, e.tasks[busy].priority)])
        _check_state(e, t)
        e.start_task_mn(m[0], [w[4], w[5]])
        assert t.assigned_add_mn([(m[0], rq_mn, 7, [w[4], w[5]])]) == 1 and t.assigned_last_unknown() == 0
        _check_state(e, t)
        cases = {
            "a busy worker": (m[1], rq_mn, [w[0], w[2]]),
            "a stopping worker": (m[1], rq_mn, [w[2], w[1]]),
            "an unknown worker": (m[1], rq_mn, [w[2], 999]),
            "a worker listed twice": (m[1], rq_mn, [w[2], w[2]]),
            "a worker that holds a multi-node task": (m[1], rq_mn, [w[2], w[5]]),
            "an id already present (multi-node)": (m[0], rq_mn, [w[2], w[3]]),
            "an id already present (single-node)": (busy, rq_mn, [w[2], w[3]]),
            "a request that is not a multi-node one": (m[1], rq_sn, [w[2], w[3]]),
            "an unknown request": (m[1], 10_000, [w[2], w[3]]),
        }
        for name, (tid, rq, ws) in cases.items():
            assert t.assigned_add_mn([(tid, rq, 1, ws)]) == 0 and t.assigned_last_unknown() == 1, name
            _check_state(e, t)
        # two tasks of one call that want the same worker: the first takes it, the second is counted; a good task beside a bad one enters
        e.start_task_mn(m[1], [w[2], w[3]])
        assert t.assigned_add_mn([(m[1], rq_mn, 1, [w[2], w[3]]), (m[2], rq_mn, 1, [w[3], 999])]) == 1 and t.assigned_last_unknown() == 1
        _check_state(e, t)
        assert t.assigned_lookup([m[1]])[0].tolist() == [w[2]]
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------- 5: hqtick_cluster_set_flags
def test_a_stopping_worker_gets_nothing_until_the_flag_is_cleared():
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB
    from hyperqueue_amd.tick import HqTickError, Tick

    cfg = abi.make_config(fill_max=0, time_limit_s=20.0)
    e = SchedEnv(cfg)
    a, b = Tick(cfg), Tick(cfg)
    try:
        w = e.new_workers_cpus([2] * 4)
        for _ in range(2):
            e.new_task(TB().n_nodes(2).user_priority(2))  # 3 free workers that are not stopping: only one of the two fits (batches.rs:65-78)
        for _ in range(10):
            e.new_task(TB().cpus(1))
        a.cluster_upload(e.snapshot()); a.assigned_enable([])
        e.workers[w[1]].stopping = True
        a.cluster_set_flags([w[1]], [SN | STOPPING])
        _check_state(e, a)
        snap = e.snapshot()
        want = _b_tick(b, snap)
        _same(_ledger_tick(a, snap), want)
        assert want.mn and not want.records[1] and all(1 not in ws for _, ws in want.mn)
        e.apply(want)
        _check_state(e, a)
        # the refusals change nothing
        for ids, fl in (([w[0]], [SN | 4]), ([999], [SN]), ([w[0], w[0]], [SN, SN]), ([w[1]], [STOPPING]), ([w[1]], [0])):
            with pytest.raises(HqTickError) as err:
                a.cluster_set_flags(ids, fl)  # (the last two would change an SN bit, which follows the ledger's multi-node tasks)
            assert err.value.code == abi.HQTICK_E_INVALID
        _check_state(e, a)
        e.workers[w[1]].stopping = False
        a.cluster_set_flags([w[1]], [SN])
        done = [tid for tid, _ in want.mn]  # the running multi-node task finishes: the waiting one no longer blocks the free workers
        for tid in done:
            _finish_mn(e, tid)
        assert a.assigned_release(done) == len(done)
        for _ in range(4):
            e.new_task(TB().cpus(1))
        _check_state(e, a)
        snap = e.snapshot()
        want = _b_tick(b, snap)
        _same(_ledger_tick(a, snap), want)
        assert want.records[1] or any(1 in ws for _, ws in want.mn)  # the worker is back
        e.apply(want)
        _check_state(e, a)
    finally:
        a.close(); b.close()


def test_set_flags_alone_drives_multi_node_tasks_without_the_ledger():
    """a resident worker set WITHOUT the ledger: the host sends free rows (hqtick_cluster_update_workers), the assigned CSR and, with
    hqtick_cluster_set_flags, what set_mn_task / reset_mn_task do to HQ_WORKER_SN"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB
    from hyperqueue_amd.tick import Tick

    cfg = abi.make_config(fill_max=0, time_limit_s=20.0)
    e = SchedEnv(cfg)
    a, b = Tick(cfg), Tick(cfg)
    try:
        e.new_workers_cpus([3] * 6)
        a.cluster_upload(e.snapshot())
        sent = np.asarray(e.snapshot().worker_flags).copy()
        placed, flag_calls = 0, 0
        for step in range(4):
            for _ in range(2):
                e.new_task(TB().n_nodes(2).user_priority(step))
            for _ in range(5):
                e.new_task(TB().cpus(1))
            snap = e.snapshot()
            W = len(snap.worker_id)
            now = np.asarray(snap.worker_flags)
            changed = np.nonzero(now != sent)[0]
            if len(changed):
                a.cluster_set_flags(snap.worker_id[changed], now[changed]); sent = now.copy(); flag_calls += 1
            assert a.cluster_worker_flags().tolist() == now.tolist()
            a.cluster_update_workers(list(range(W)), np.asarray(snap.worker_free, np.uint64).reshape(W, -1))
            want = _b_tick(b, snap)
            got = abi.parse_result(a.tick_raw(snap.to_c(resident_workers=True)), W, snap.n_resources)
            _same(got, want)
            placed += len(want.mn)
            e.apply(want)
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state == RUNNING_MN and (t.id + step) % 2 == 0:
                    _finish_mn(e, t.id)
                elif t.state in (ASSIGNED, RUNNING) and t.id % 3 == 0:
                    e.finish_task(t.id, t.worker)
        assert placed >= 2 and flag_calls >= 1, (placed, flag_calls)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 6: consume forms and record forms
def _mn_env():
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB

    e = SchedEnv(abi.make_config(fill_max=0, time_limit_s=20.0))
    e.new_workers_cpus([4] * 7)
    e.new_task(TB().n_nodes(2).user_priority(4)); e.new_task(TB().n_nodes(3).user_priority(2))
    for i in range(20):
        e.new_task(TB().cpus(1 + i % 2))
    return e


def _resident_ctx(snap, flags=0, sink=False):
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import Tick
    from test_gpu_assigned_forms import Sink

    t = Tick(abi.make_config(fill_max=0, time_limit_s=20.0, flags=flags))
    t.cluster_upload(snap)
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    t.assigned_enable([])
    return t, (Sink(t, sink_layout(len(snap.worker_id), 4096)[4]) if sink else None)


def _resident_tick(t, snap, sink=None):
    from test_gpu_assigned_forms import _parse

    return _parse(t.tick_raw(_strip(snap.to_c(resident_workers=True)), resident=True), len(snap.worker_id), snap.n_resources, sink)


def _mn_view(t, res, snap):
    ids = snap.worker_id.tolist()
    for tid, ws in res.mn:
        assert t.assigned_mn_workers(tid) == [ids[ws[0]]] + sorted(ids[k] for k in ws[1:])
    return t.cluster_worker_flags().tolist(), t.assigned_mn_count(), t.assigned_count(), t.assigned_free_rows().tolist()


def test_every_consume_form_and_record_form_enters_the_multi_node_placement():
    from hyperqueue_amd.tick import HqTickError

    e = _mn_env()
    snap = e.snapshot()
    W = len(snap.worker_id)
    in_tick, compact = abi.HQTICK_FLAG_CONSUME_IN_TICK, abi.HQTICK_FLAG_COMPACT_RECORDS
    ctxs = [_resident_ctx(snap), _resident_ctx(snap, in_tick), _resident_ctx(snap, in_tick, sink=True), _resident_ctx(snap, compact)]
    try:
        res = []
        for i, (t, sink) in enumerate(ctxs):
            res.append(_resident_tick(t, snap, sink))
            if i in (0, 3):  # the two-call form: nothing has entered yet, and ledger calls wait for the consume
                assert t.assigned_mn_count() == 0 and t.cluster_worker_flags().tolist() == [SN] * W
                with pytest.raises(HqTickError) as err:
                    t.cluster_set_flags([int(snap.worker_id[0])], [SN | STOPPING])
                assert err.value.code == abi.HQTICK_E_INVALID
                t.ready_consume_last()
        for r in res[1:]:
            assert r.mn == res[0].mn and r.records == res[0].records
        assert len(res[0].mn) == 2
        views = [_mn_view(t, r, snap) for (t, _), r in zip(ctxs, res)]
        assert views[0] == views[1] == views[2] == views[3]
        listed = sorted(k for _, ws in res[0].mn for k in ws)
        assert [i for i in range(W) if not views[0][0][i] & SN] == listed and views[0][1] == 2
        # and out again, mixed with the single-node tasks, on every context
        run = [x[0] for w in res[0].records for x in w if x[2] == abi.HQ_REC_ASSIGN][::2] + [tid for tid, _ in res[0].mn]
        for t, _ in ctxs:
            assert t.assigned_release(run) == len(run) and t.assigned_mn_count() == 0 and t.cluster_worker_flags().tolist() == [SN] * W
    finally:
        for t, _ in ctxs:
            t.close()


def test_an_abandoned_two_call_tick_enters_no_multi_node_task():
    e = _mn_env()
    snap = e.snapshot()
    W = len(snap.worker_id)
    t, _ = _resident_ctx(snap)
    try:
        r = _resident_tick(t, snap)
        assert len(r.mn) == 2
        top = int(snap.task_id.max()) + 1
        t.ready_add_packed([(top, 4)], [(0, 4)], np.full(4, 2, np.uint16))  # a ready-set delta (four more cpus(1) tasks) drops the tick's selection
        t.ready_consume_last()
        assert t.assigned_mn_count() == 0 and t.assigned_count() == 0 and t.cluster_worker_flags().tolist() == [SN] * W
        assert all(t.assigned_mn_workers(tid) == [] for tid, _ in r.mn)
        r2 = _resident_tick(t, snap)  # the next tick places them again, and this time the placement enters
        t.ready_consume_last()
        assert len(r2.mn) == 2 and t.assigned_mn_count() == 2
        flags = t.cluster_worker_flags().tolist()
        assert [i for i in range(W) if not flags[i] & SN] == sorted(k for _, ws in r2.mn for k in ws)
    finally:
        t.close()


def test_a_lost_root_goes_back_into_the_resident_ready_set():
    e = _mn_env()
    snap = e.snapshot()
    W = len(snap.worker_id)
    ids = snap.worker_id.tolist()
    meta = {int(t): (int(q), int(p)) for t, q, p in zip(snap.task_id, snap.task_rq, snap.task_priority)}
    t, _ = _resident_ctx(snap, abi.HQTICK_FLAG_CONSUME_IN_TICK)
    try:
        r = _resident_tick(t, snap)
        (tid, ws) = max(r.mn, key=lambda x: len(x[1]))  # the 3-node task
        live = t.ready_count()
        assert t.cluster_remove_workers([ids[ws[0]]]) == []
        assert t.cluster_last_requeued() == [(tid, meta[tid][0], meta[tid][1])]
        assert t.ready_count() == live + 1 and t.assigned_mn_count() == 1 and t.assigned_mn_workers(tid) == []
        assert t.ready_remove([tid]) == 1  # it is in the ready set
        flags = t.cluster_worker_flags().tolist()
        left = [w for w in ids if w != ids[ws[0]]]
        other = [k for x, ks in r.mn if x != tid for k in ks]
        assert [left[i] for i in range(W - 1) if not flags[i] & SN] == sorted(ids[k] for k in other)
    finally:
        t.close()
