"""task_finished scenarios on SchedEnv, shared by tests/test_finish_oracle.py (the mirror alone, the CPU oracle as the scheduler) and tests/test_gpu_finish.py (the
same scenarios through hqtick_finish_tasks / hqtick_retracting_started).  The reference's outcomes are restated from tests/test_reactor.rs: the finish part of
test_assignments_and_finish (:199), test_steal_finished (:1009), test_steal_running (:1022), and a multi-node finish reported by the root built the way
cancel_cases.scenario_mn_cancel builds its task.  Not a test module."""
from __future__ import annotations

import cancel_cases as cc
from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB

K = abi


def scenario_assignments_and_finish():
    """test_reactor.rs:199-275: workers of 2, 3 and 1 cpus; t1, t5 on ws[0], t2 on ws[1] (the placement the reference's tick makes, :223-245), t3 waits for t1 and
    t2, t7 for t4.  Three single-position batches: t5 by ws[0] (:247), t2 by ws[1] (:261), t1 by ws[0] (:272).  After each the finished task is gone and the
    workers hold exactly what the reference's check_worker_tasks_exact lists (:250-252, :264-266); scheduling is asked for every time (:254, :268, :274); after
    the last one t3 is ready (the next tick assigns it, :279-286).
    -> (mirror, workers, [(pairs, {worker: tasks it still holds}, released consumers)], tasks)"""
    e = SchedEnv()
    ws = e.new_workers_cpus([2, 3, 1])
    t1 = e.new_task(TB().user_priority(12).cpus(1)); t2 = e.new_task(TB().user_priority(12).cpus(3))
    t3 = e.new_task(TB().user_priority(12).cpus(1).task_deps([t1, t2]))
    t4 = e.new_task(TB().cpus(3)); t5 = e.new_task(TB().user_priority(12).cpus(1)); t7 = e.new_task(TB().task_deps([t4]))
    e.assign_task(t1, ws[0]); e.assign_task(t5, ws[0]); e.assign_task(t2, ws[1])
    steps = [([(t5, ws[0])], {ws[0]: {t1}, ws[1]: {t2}, ws[2]: set()}, []),
             ([(t2, ws[1])], {ws[0]: {t1}, ws[1]: set(), ws[2]: set()}, []),
             ([(t1, ws[0])], {ws[0]: set(), ws[1]: set(), ws[2]: set()}, [t3])]
    return e, ws, steps, dict(t1=t1, t2=t2, t3=t3, t4=t4, t5=t5, t7=t7)


def scenario_mn_finish():
    """a three-node task on workers 3, 1, 0 of four, finished by its ROOT (reactor.rs:543-546: assert_eq!(ws[0], worker_id), reset_mn_task_workers): every worker
    is free and single-node again; a finish reported by a non-root worker is what the reference asserts against.  -> (mirror, task, root, a non-root worker)"""
    e, ids, want, survivors = cc.scenario_mn_cancel()
    (t1,) = ids
    (root,) = want
    return e, t1, root, e.tasks[t1].mn_workers[1]


def scenario_steal(backend):
    """setup_retracting (test_reactor.rs:993-1007) as cancel_cases.scenario_steal_cancel builds it: t is Retracting{w1} with a redirect to w2, one task is assigned
    on w1, one on w2.  -> (mirror, w1, w2, t, the task assigned on w1)"""
    e, ids, want, survivors, w2 = cc.scenario_steal_cancel(backend)
    (t,) = ids
    (w1,) = want
    (on_w1,) = sorted(e.workers[w1].assigned_tasks)
    return e, w1, w2, t, on_w1


def check_steal_finished(e: SchedEnv, w1, w2, t, free_w2_before):
    """test_steal_finished (:1009-1019): the task is gone (:1017), the redirect is gone with the target's resources free again (try_remove_redirection,
    reactor.rs:599-603; sanity_check :1018 counts a Retracting task on its target), scheduling was asked for (:1015: the batch accepted a position)"""
    assert e.tasks[t].state == core.FINISHED and t not in e.redirects
    assert t not in e.workers[w2].assigned_tasks and e.workers[w2].free[0] == free_w2_before + core.amount(1)
    assert all(t not in s for s in e.ready.values())
    assert e.last_finish_kinds == [K.HQ_FINISH_RETRACTING]


def check_steal_running(e: SchedEnv, w1, w2, t, on_w1):
    """test_steal_running (:1022-1047): after Finished(the task assigned on w1) and Running(t), both from w1, t is Running on w1 (:1041-1046) -- inserted there
    after its redirect's entry on w2 was removed (reactor.rs:315-333)"""
    assert e.tasks[on_w1].state == core.FINISHED
    x = e.tasks[t]
    assert x.state == core.RUNNING and x.worker == w1 and t not in e.redirects
    assert e.workers[w1].assigned_tasks == {t} and t not in e.workers[w2].assigned_tasks
