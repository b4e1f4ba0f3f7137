"""task_running / on_remove_worker scenarios on SchedEnv, shared by tests/test_start_oracle.py (the mirror alone, the CPU oracle as the scheduler) and
tests/test_gpu_start.py (the same scenarios through hqtick_start_tasks, hqtick_assigned_running and hqtick_cluster_last_requeued_running).  The reference's outcomes
are restated from tests/test_reactor.rs: test_running_task (:524), lost_worker_with_running_and_assign_tasks (:572), test_prefill_started_on_same_worker (:866),
test_prefill_started (:905), test_steal_running (:1022) and test_worker_lost_with_mn_task_root (:413).  Not a test module."""
from __future__ import annotations

import cancel_cases as cc
import finish_cases as fc
from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

K = abi


def scenario_running_task():
    """test_running_task (:524-569): three 10-cpu workers, t1 and t2 assigned on ws[1]; Running(t1), then Running(t2), both from ws[1]: both are Running there
    (:544-557); ws[1] is lost: the client hears [t1, t2] (:559-562).  -> (mirror, workers, t1, t2)"""
    e = SchedEnv()
    ws = e.new_workers_cpus([10, 10, 10])
    t1 = e.new_task_assigned(TB(), ws[1]); t2 = e.new_task_assigned(TB(), ws[1])
    return e, ws, t1, t2


def check_running_task(e: SchedEnv, ws, t1, t2):
    for t in (t1, t2):
        assert e.tasks[t].state == core.RUNNING and e.tasks[t].worker == ws[1]


def scenario_lost_worker():
    """lost_worker_with_running_and_assign_tasks (:572-606): the diamond and two more tasks; wf[0] and t1 assigned on ws[1], wf[1] assigned there too and then
    reported running (assign_and_start_task, :581).  ws[1] is lost: the client hears [wf[1]] only (:590); wf[0], wf[1] and t1 are ready again (:592-595).
    -> (mirror, workers, the diamond, t1, t2, the start batch)"""
    e = SchedEnv()
    ws = e.new_workers_cpus([10, 10, 10])
    wf = cc.diamond(e)
    t1, t2 = e.new_task(), e.new_task()
    e.assign_task(wf[0], ws[1]); e.assign_task(wf[1], ws[1]); e.assign_task(t1, ws[1])
    return e, ws, wf, t1, t2, [(wf[1], ws[1], 0)]


def check_lost_worker(e: SchedEnv, ws, wf, t1, t2):
    assert e.last_lost_running == [wf[1]]
    for t in (wf[0], wf[1], t1, t2):
        assert e.tasks[t].state == core.WAITING and t in e.ready[e.tasks[t].rq]


def scenario_prefill_started(backend):
    """test_prefill_started (:905-930): setup_prefill; Finished(t1) and RunningPrefilled(t2) from w1: t2 is Running on w1 (:915-920), the worker's prefilled set
    is empty (:922-928).  -> (mirror, w1, the assigned task, the prefilled task)"""
    e, w1, tasks, assigned, prefilled = cc.setup_prefill(backend)
    return e, w1, assigned, prefilled


def check_prefill_started(e: SchedEnv, w1, assigned, prefilled):
    x = e.tasks[prefilled]
    assert x.state == core.RUNNING and x.worker == w1 and e.tasks[assigned].state == core.FINISHED
    assert not e.workers[w1].prefilled_tasks and e.workers[w1].assigned_tasks == {prefilled}
    assert e.last_start_kinds == [K.HQ_START_PREFILLED]


def setup_same_worker(e: SchedEnv, schedule):
    """test_prefill_started_on_same_worker (:866-902) up to the Running message: reserve 0, at most 3 prefilled; t1 on the 2-cpu worker w1; two more tasks, one
    assigned, one prefilled; t1 finishes and the next tick takes the prefilled task for w1 itself: it is Retracting{w1} (:897).  schedule(): one tick applied to
    the mirror.  -> (w1, t1, the assigned task, the Retracting task)"""
    t1 = e.new_task()
    w1 = e.new_worker(WB(2))
    schedule()
    assert e.task(t1).is_assigned()
    tasks = e.new_tasks(2, TB())
    schedule()
    prefilled = next(t for t in tasks if e.task(t).is_prefilled())
    assigned = next(t for t in tasks if e.task(t).is_assigned())
    return w1, t1, assigned, prefilled


def check_same_worker(e: SchedEnv, w1, prefilled):
    """after Running(prefilled) from w1 (:899-901): the Retracting arm ran -- the task runs on w1 and is in no redirect, no queue and no prefill set"""
    x = e.tasks[prefilled]
    assert x.state == core.RUNNING and x.worker == w1 and prefilled in e.workers[w1].assigned_tasks
    assert prefilled not in e.redirects and prefilled not in e.retaken_variant and all(prefilled not in s for s in e.ready.values())
    assert e.last_start_kinds == [K.HQ_START_RETRACTING]


scenario_steal = fc.scenario_steal          # test_steal_running (:1022-1047): Finished(the task on w1), then Running(t), both from w1
check_steal_running = fc.check_steal_running


def scenario_mn_root():
    """test_worker_lost_with_mn_task_root (:413-430): a three-node task on workers 3, 1, 0 of four; the root is lost: the task is Waiting again (:429), and it is the
    one task the client hears of.  -> (mirror, task, root, a non-root worker)"""
    return fc.scenario_mn_finish()
