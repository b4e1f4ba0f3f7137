"""task_failed scenarios on SchedEnv, shared by tests/test_fail_oracle.py (the mirror alone, the CPU oracle as the scheduler) and tests/test_gpu_fail.py (the same
scenarios through hqtick_fail_tasks).  The reference's outcomes are restated from tests/test_reactor.rs: test_running_task_on_error (:308), test_task_mn_fail
(:472), test_prefill_failed (:950), test_steal_failed (:1051) and the crash-limit path of test_worker_crashing_task (:433).  Also the random histories both
files run, and what a history must contain to be worth running.  Not a test module."""
from __future__ import annotations

import numpy as np

import cancel_cases as cc
from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

K = abi
NO = abi.HQ_NO_WORKER
HISTORY_SEEDS = range(20)
CFG = dict(time_limit_s=20.0)


def scenario_running_task_on_error():
    """test_reactor.rs:308-345: three 1-cpu workers, submit_example_1 (workflows.rs: 0 and 1 feed 2, 1 feeds 3, 2 and 3 feed 4, 2 feeds 5, 5 feeds 6); wf[0] and
    wf[1] have finished, wf[2] is assigned on ws[2] and fails there.  The client is told wf[2] with the consumers {wf[4], wf[5], wf[6]} (:333-335); the worker
    no longer holds it (:331); wf[4] and wf[5] are gone (:339-340); wf[3] survives.  -> (mirror, ws, wf)"""
    e = SchedEnv(abi.make_config(**CFG))
    ws = e.new_workers_cpus([1, 1, 1])
    wf = cc.diamond(e)
    for x, w in ((wf[0], ws[0]), (wf[1], ws[1])):  # start_and_finish_task
        e.assign_and_start_task(x, w)
        e.finish_tasks([(x, w)])
    e.assign_task(wf[2], ws[2])
    return e, ws, wf


def check_running_task_on_error(e: SchedEnv, ws, wf):
    assert e.last_fail_kinds == [K.HQ_FAIL_ASSIGNED] and e.last_fail_consumers == [[wf[4], wf[5], wf[6]]]
    assert wf[2] not in e.workers[ws[2]].assigned_tasks and e.workers[ws[2]].free == e.workers[ws[2]].total
    assert all(e.tasks[x].state == core.FINISHED for x in (wf[2], wf[4], wf[5], wf[6]))
    assert e.tasks[wf[3]].state == core.WAITING and wf[3] in e.ready[e.tasks[wf[3]].rq]


def scenario_mn_fail():
    """test_reactor.rs:472-494 on cancel_cases.scenario_mn_cancel's task: a three-node task on workers 3, 1, 0 of four fails, reported by its root; the task is gone
    (:490) and no worker holds a multi-node assignment (:491-493).  -> (mirror, task, root, a non-root worker)"""
    e, ids, want, survivors = cc.scenario_mn_cancel()
    (t1,) = ids
    (root,) = want
    return e, t1, root, e.tasks[t1].mn_workers[1]


def check_mn_fail(e: SchedEnv, t1):
    assert e.tasks[t1].state == core.FINISHED and all(w.mn_task is None for w in e.workers.values())


def check_prefill_failed(e: SchedEnv, w1, t1, t2):
    """test_prefill_failed (:950-975): after Finished(t1) and Failed(t2), both from w1, neither task exists (:964-965), the worker is free (:966) and its
    prefilled set is empty (:967-973)"""
    assert e.tasks[t1].state == core.FINISHED and e.tasks[t2].state == core.FINISHED
    w = e.workers[w1]
    assert not w.assigned_tasks and not w.prefilled_tasks and w.free == w.total
    assert e.last_fail_kinds == [K.HQ_FAIL_PREFILLED] and e.last_fail_consumers == [[]]
    assert all(t2 not in s for s in e.ready.values()) and all(t2 not in s[1] for s in e.prefill.values())


def check_steal_failed(e: SchedEnv, w1, w2, t, free_w2_before):
    """test_steal_failed (:1051-1075): after Finished(the task assigned on w1) and Failed(t), both from w1, t is gone (:1073) and the redirect with it: the
    target's resources are free again (try_remove_redirection, reactor.rs:592-604; sanity_check :1074 counts a Retracting task on its redirect target)"""
    assert e.tasks[t].state == core.FINISHED and t not in e.redirects
    assert t not in e.workers[w2].assigned_tasks and e.workers[w2].free[0] == free_w2_before + core.amount(1)
    assert all(t not in s for s in e.ready.values())
    assert e.last_fail_kinds == [K.HQ_FAIL_RETRACTING]


def scenario_crash_limit():
    """the last round of test_worker_crashing_task (:433-468): t1 runs on a worker that is lost; on_remove_worker puts it back into its queue (reactor.rs:130-160)
    and, the crash limit reached, fails it with task_failed(None, ..) (:164-183): the task is gone, nobody was holding it.  -> (mirror, worker, task)"""
    e = SchedEnv(abi.make_config(**CFG))
    t1 = e.new_task(TB())
    w = e.new_worker(WB(1))
    e.new_worker(WB(1))  # (a second, idle worker: the resident worker set is never left empty)
    e.assign_and_start_task(t1, w)
    return e, w, t1


# ---------------------------------------------------------------------------------------------- attribution shapes
def shapes():
    """name -> (mirror, pairs): graphs at the smallest sizes at which the attribution can go wrong.  Roots are assigned on one wide worker and fail by it unless
    said otherwise."""
    out = {}

    def env():
        e = SchedEnv(abi.make_config(**CFG))
        return e, e.new_workers_cpus([600, 600])

    # two roots share a consumer; the larger position's root is listed first in the graph (the smaller id)
    e, ws = env()
    r0, r1 = e.new_task(TB().cpus(1)), e.new_task(TB().cpus(1))
    e.new_task(TB().cpus(1).task_deps([r0, r1])); e.new_task(TB().cpus(1).task_deps([r0])); e.new_task(TB().cpus(1).task_deps([r1]))
    e.assign_task(r0, ws[0]); e.assign_task(r1, ws[0])
    out["shared_consumer"] = (e, [(r1, ws[0]), (r0, ws[0])])

    # a task first reached at depth 2 from position 1 and at depth 3 from position 0: it and what it reaches belong to position 0
    e, ws = env()
    a, b = e.new_task(TB().cpus(1)), e.new_task(TB().cpus(1))
    a1 = e.new_task(TB().cpus(1).task_deps([a])); a2 = e.new_task(TB().cpus(1).task_deps([a1]))
    b1 = e.new_task(TB().cpus(1).task_deps([b]))
    x = e.new_task(TB().cpus(1).task_deps([a2, b1])); e.new_task(TB().cpus(1).task_deps([x])); e.new_task(TB().cpus(1).task_deps([b1]))
    e.assign_task(a, ws[0]); e.assign_task(b, ws[1])
    out["relabel_depth_2_vs_3"] = (e, [(a, ws[0]), (b, ws[1])])

    # a chain of 70 under one root (more levels than a wavefront has lanes), a second root joining it half way with a smaller position
    e, ws = env()
    r = e.new_task(TB().cpus(1)); late = e.new_task(TB().cpus(1))
    chain = [r]
    for k in range(70):
        chain.append(e.new_task(TB().cpus(1).task_deps([chain[-1]] + ([late] if k == 35 else []))))
    e.assign_task(r, ws[0]); e.assign_task(late, ws[1])
    out["chain_of_70"] = (e, [(late, ws[1]), (10**12, ws[0]), (r, ws[0])])

    # a root with 300 direct consumers (crossing a 256-thread workgroup), every third one shared with a root at a smaller position
    e, ws = env()
    wide, other = e.new_task(TB().cpus(1)), e.new_task(TB().cpus(1))
    for k in range(300):
        e.new_task(TB().cpus(1).task_deps([wide, other] if k % 3 == 0 else [wide]))
    e.assign_task(wide, ws[0]); e.assign_task(other, ws[0])
    out["fan_of_300"] = (e, [(other, ws[0]), (wide, ws[0])])

    # a _WAITING root inside an earlier root's closure becomes _GONE, one inside a LATER root's closure is accepted and owns what it reaches
    e, ws = env()
    r0, r1 = e.new_task(TB().cpus(1)), e.new_task(TB().cpus(1))
    g = e.new_task(TB().cpus(1).task_deps([r0])); e.new_task(TB().cpus(1).task_deps([g]))
    h = e.new_task(TB().cpus(1).task_deps([r1])); e.new_task(TB().cpus(1).task_deps([h]))
    lone = e.new_task(TB().cpus(1))
    e.assign_task(r0, ws[0]); e.assign_task(r1, ws[1])
    out["waiting_root_gone"] = (e, [(h, NO), (r0, ws[0]), (g, NO), (r1, ws[1]), (lone, NO), (lone, NO), (lone, ws[0]), (r0, NO)])

    # batch sizes at wave and workgroup edges: alternating accepted and refused positions, every accepted root with two consumers, one shared with its neighbour
    for n in (1, 63, 64, 65, 256, 257):
        e, ws = env()
        roots = [e.new_task(TB().cpus(1)) for _ in range(n)]
        for k, r in enumerate(roots):
            e.new_task(TB().cpus(1).task_deps([r])); e.new_task(TB().cpus(1).task_deps([r, roots[(k + 2) % n]] if n > 2 else [r]))
        for k, r in enumerate(roots):
            e.assign_task(r, ws[k % 2])
        out["batch_of_%d" % n] = (e, [(r, ws[(k + (k % 2)) % 2]) for k, r in enumerate(roots)])  # odd positions: the wrong worker
    return out


# ---------------------------------------------------------------------------------------------- random histories
def history(seed: int):
    """a mirror with a layered DAG whose source tasks are held in every way a task can be (assigned, running, multi-node, prefilled, Retracting in its queue) and
    one fail batch that reports them rightly, wrongly, twice, by HQ_NO_WORKER, together with waiting tasks failed by the server and by workers, and unknown ids.
    Built by hand on the mirror (no tick), so that the CPU suite sees exactly the batches the GPU suite runs.  -> (mirror, pairs)"""
    rng = np.random.default_rng(7300 + seed)
    e = SchedEnv(abi.make_config(reserve=1, fill_max=2, **CFG))
    ws = [e.new_worker(WB(64)) for _ in range(int(rng.integers(2, 4)))]
    mn_ws = [e.new_worker(WB(1)) for _ in range(2)]
    pf_w = e.new_worker(WB(16))  # the prefilled tasks' worker: one prefill set per request, one worker
    shapes_ = [TB().cpus(1), TB().cpus(2), TB().cpus(3).next_variant().cpus(1)]
    src = [e.new_task(shapes_[int(rng.integers(0, 3))]) for _ in range(24)]
    pf_src = [e.new_task(TB().cpus(1).user_priority(-3)) for _ in range(2)]
    mn = e.new_task(TB().n_nodes(2))
    tasks = src + pf_src + [mn]
    for _ in range(45):
        deps = [tasks[int(k)] for k in rng.choice(len(tasks), int(rng.integers(1, 3)), replace=False)]
        tasks.append(e.new_task(shapes_[int(rng.integers(0, 3))].task_deps(deps)))
    e.start_task_mn(mn, [mn_ws[1], mn_ws[0]])
    retracting = []
    for x in src:
        u = rng.random()
        w = ws[int(rng.integers(0, len(ws)))]
        if u < 0.35:
            e.assign_task(x, w, 0)
        elif u < 0.6:
            e.assign_and_start_task(x, w, 0)
        elif u < 0.68 and len(retracting) < 2:  # process_retracted's leftovers: in its queue, no redirect
            tk = e.tasks[x]; tk.state, tk.worker = core.RETRACTING, w
            retracting.append(x)
    for x in pf_src:
        y = e.tasks[x]; y.state, y.worker = core.PREFILLED, pf_w
        e.workers[pf_w].prefilled_tasks.add(x); e.ready[y.rq].discard(x)
        if y.rq not in e.prefill:
            e.prefill[y.rq] = (y.priority, core.task_id_set())
        e.prefill[y.rq][1].insert(x)
    everyone = ws + mn_ws + [pf_w]
    pairs = []
    for x in tasks:
        tk = e.tasks[x]
        u = rng.random()
        if tk.state == core.WAITING:
            if u < 0.10:
                pairs.append((x, NO))
            elif u < 0.14:
                pairs.append((x, everyone[int(rng.integers(0, len(everyone)))]))
            continue
        if u > 0.55:
            continue
        right = tk.mn_workers[0] if tk.state == core.RUNNING_MN else tk.worker
        v = rng.random()
        pairs.append((x, right if v < 0.75 else NO if v < 0.85 else everyone[int(rng.integers(0, len(everyone)))]))
    pairs += [pairs[int(rng.integers(0, len(pairs)))] for _ in range(len(pairs) // 4)]
    pairs += [(10**12 + seed, ws[0]), (10**12 + 100 + seed, NO)]
    pairs = [pairs[int(k)] for k in rng.permutation(len(pairs))]
    return e, pairs


def seed_context(t, e: SchedEnv, graph=True):
    """worker set, ledger with prefilled tracking, Retracting table (in-queue tasks without a redirect, as process_retracted leaves them), ready set and graph of
    context t from the mirror"""
    retr = [x for x in e.tasks.values() if x.state == core.RETRACTING]
    assert not any(x.id in e.redirects for x in retr)
    for x in retr:
        x.state = core.WAITING
    try:
        cc.seed_ledger(t, e)
    finally:
        for x in retr:
            x.state = core.RETRACTING
    if retr:
        t.retracting_add([x.id for x in retr], [x.worker for x in retr])
    cc.seed_ready_graph(t, e, graph=graph)


def depths_from(e: SchedEnv, root: int):
    """{task: depth} of the transitive consumers of root among the tasks that are still here (BFS)"""
    depth, frontier, d = {}, [root], 0
    while frontier:
        d += 1
        nxt = []
        for x in frontier:
            for c in e.tasks[x].consumers:
                if c not in depth and c != root and e.tasks[c].state != core.FINISHED:
                    depth[c] = d; nxt.append(c)
        frontier = nxt
    return depth


def owner_is_not_the_nearest(depth_of_root: dict, kinds, consumers):
    """whether some consumer belongs to a position although ANOTHER accepted position's root reaches it in fewer steps: the case a first-writer-wins BFS gets
    wrong.  depth_of_root: position -> depths_from of its root on the state BEFORE the batch."""
    acc = [i for i, k in enumerate(kinds) if k in K.HQ_FAIL_ACCEPTED]
    for i in acc:
        for c in consumers[i]:
            if any(j != i and depth_of_root[j].get(c, 1 << 30) < depth_of_root[i][c] for j in acc):
                return True
    return False
