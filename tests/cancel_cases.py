"""on_cancel_tasks scenarios on SchedEnv, shared by tests/test_cancel_oracle.py (the mirror alone, the CPU oracle as the scheduler) and tests/test_gpu_cancel.py (the
same scenarios through hqtick_cancel_tasks).  The four reference scenarios are tests/test_reactor.rs's test_task_cancel (:359), test_task_mn_cancel (:497),
test_prefill_cancel (:978) and test_steal_cancel (:1078), restated here with the outcomes the reference asserts.  Not a test module."""
from __future__ import annotations

import numpy as np

from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

LIVE = (core.WAITING, core.ASSIGNED, core.RUNNING, core.PREFILLED, core.RETRACTING, core.RUNNING_MN)


def diamond(e: SchedEnv):
    """workflows.rs submit_example_1: 0 and 1 feed 2, 1 feeds 3, 2 and 3 feed 4, 2 feeds 5, 5 feeds 6"""
    t0 = e.new_task(); t1 = e.new_task()
    t2 = e.new_task(TB().task_deps([t0, t1])); t3 = e.new_task(TB().task_deps([t1]))
    t4 = e.new_task(TB().task_deps([t2, t3])); t5 = e.new_task(TB().task_deps([t2])); t6 = e.new_task(TB().task_deps([t5]))
    return [t0, t1, t2, t3, t4, t5, t6]


def scenario_task_cancel():
    """three 10-cpu workers, the diamond, three more tasks; four of them assigned; five ids cancelled -> worker 0 is told [t2], worker 1 {wf0, wf1, t1}, t3 survives"""
    e = SchedEnv()
    ws = e.new_workers_cpus([10, 10, 10])
    wf = diamond(e)
    t1, t2, t3 = e.new_task(), e.new_task(), e.new_task()
    e.assign_task(wf[0], ws[1]); e.assign_task(wf[1], ws[1]); e.assign_task(t1, ws[1]); e.assign_task(t2, ws[0])
    return e, [wf[0], wf[1], t1, t2, wf[2]], {ws[0]: [t2], ws[1]: [wf[0], wf[1], t1]}, [t3]


def scenario_mn_cancel():
    """a three-node task on workers 3, 1, 0 of four: only its root (worker 3) is told, every worker is free again"""
    e = SchedEnv()
    ws = e.new_workers_cpus([1, 1, 1, 1])
    t1 = e.new_task(TB().n_nodes(3))
    e.start_task_mn(t1, [ws[3], ws[1], ws[0]])
    return e, [t1], {ws[3]: [t1]}, []


def setup_prefill(backend):
    """test_reactor.rs:775-795: reserve 1, at most one prefilled task; three tasks, one 1-cpu worker, one tick: one assigned, one prefilled, one waiting"""
    e = SchedEnv(abi.make_config(reserve=1, fill_max=1, time_limit_s=20.0))
    tasks = e.new_tasks(3, TB())
    w1 = e.new_worker(WB(1))
    e.schedule(backend)
    assigned = next(t for t in tasks if e.task(t).is_assigned())
    prefilled = next(t for t in tasks if e.task(t).is_prefilled())
    return e, w1, tasks, assigned, prefilled


def scenario_prefill_cancel(backend):
    """the prefilled task cancelled: its worker is told, the assigned task stays"""
    e, w1, tasks, assigned, prefilled = setup_prefill(backend)
    return e, [prefilled], {w1: [prefilled]}, [t for t in tasks if t != prefilled]


def scenario_steal_cancel(backend):
    """test_reactor.rs:993-1007: a second worker of 2 cpus joins and the next tick takes the prefilled task for it: Retracting{w1} with a redirect to w2.
    Cancelled: the worker it is retracting FROM is told."""
    e, w1, tasks, assigned, prefilled = setup_prefill(backend)
    w2 = e.new_worker(WB(2))
    e.schedule(backend)
    t = next(t for t in tasks if e.task(t).is_retracting())
    assert e.task(t).worker == w1 and e.redirects[t][0] == w2
    return e, [t], {w1: [t]}, [x for x in tasks if x != t], w2


def check_outcome(e: SchedEnv, messages, want, survivors):
    assert messages == want
    assert sorted(t for t, x in e.tasks.items() if x.state != core.FINISHED) == sorted(survivors)
    for s in e.ready.values():
        assert all(e.tasks[t].state != core.FINISHED for t in s)


# ---------------------------------------------------------------------------------------------- SchedEnv -> a context's resident state
def live_tasks(e: SchedEnv):
    return [t for t in sorted(e.tasks.values(), key=lambda t: t.id) if t.state in LIVE]


def seed_ledger(t, e: SchedEnv):
    """worker set, ledger and prefilled tracking of context t from the mirror's Assigned / Running / RunningMultiNode / Prefilled tasks (no Retracting ones: those
    come out of ticks)"""
    t.cluster_upload(e.snapshot())
    live = live_tasks(e)
    assert not any(x.state == core.RETRACTING for x in live)
    t.assigned_enable([(x.id, x.worker, x.rq, x.rv, x.priority) for x in live if x.state in (core.ASSIGNED, core.RUNNING)])
    mn = [(x.id, x.rq, x.priority, list(x.mn_workers)) for x in live if x.state == core.RUNNING_MN]
    if mn:
        assert t.assigned_add_mn(mn) == len(mn)
    pf = [(x.id, x.worker, x.rq, x.priority) for x in live if x.state == core.PREFILLED]
    assert t.assigned_track_prefilled(pf) == len(pf)


def seed_ready_graph(t, e: SchedEnv, graph=True):
    """the resident ready set (and, with graph, every live task in the dependency graph) of context t from the mirror"""
    t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    ready = sorted(x for s in e.ready.values() for x in s)
    if not graph:
        t.ready_add(ready, [e.tasks[x].priority for x in ready], [e.tasks[x].rq for x in ready])
        return
    live = live_tasks(e)
    ids = {x.id for x in live}
    producers = {}
    for x in live:
        for c in x.consumers:
            producers.setdefault(c, []).append(x.id)
    now = t.graph_add_tasks([x.id for x in live], [x.priority for x in live], [x.rq for x in live], [sorted(producers.get(x.id, [])) for x in live])
    assert set(now.tolist()) == {x.id for x in live if x.unfinished_deps == 0}
    placed = sorted(set(now.tolist()) - set(ready))  # released by the graph, but Assigned / Running / Prefilled / ... in the mirror: not in a queue
    if placed:
        assert t.ready_remove(placed) == len(placed)
    assert t.ready_count() == len(ready) and ids >= set(ready)


def free_rows(e: SchedEnv):
    snap = e.snapshot()
    return np.asarray(snap.worker_free, np.uint64).reshape(len(snap.worker_id), snap.n_resources)
