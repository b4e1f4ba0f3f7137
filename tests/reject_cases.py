"""task_reject / request_enabled scenarios on SchedEnv, shared by tests/test_reject_oracle.py (the mirror alone, the CPU oracle as the scheduler) and
tests/test_gpu_reject.py (the same through hqtick_reject_tasks, hqtick_cluster_enable_request and hqtick_cluster_blocked).  The reference's outcomes are restated
from tests/test_reactor.rs: test_task_reject1 (:665-705), test_task_reject2 (:708-734), test_task_reject3 (:737-773), test_prefill_rejected (:933-947) and
test_steal_rejected (:1119-1138).  Each scenario's setup differs by side (the mirror's scheduler is the oracle, a context's is the context); what follows the setup
is written once, against a `side`:
    side.schedule()            one tick, applied to the mirror
    side.reject(triples)       the batch on the mirror (and the context) -> the kinds
    side.enable(w, rq, v)      request_enabled -> 1 if the pair was blocked
And seeded histories: lifecycle_cases.History with reject batches and enable-requests drawn between its other steps.  Not a test module."""
from __future__ import annotations

import lifecycle_cases as lc
from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB

K = abi
NONE_V = None  # a RejectRequest that names no variant
GHOST = 4000   # a worker id no history's worker set holds


class MirrorSide:
    """the scenarios on the mirror alone; backend: the scheduler"""

    def __init__(self, e: SchedEnv, backend):
        self.e, self.backend = e, backend

    def schedule(self):
        self.e.schedule(self.backend)

    def reject(self, triples):
        self.e.reject_tasks(triples)
        return list(self.e.last_reject_kinds)

    def enable(self, wid, rq, v):
        was = (rq, v) in self.e.workers[wid].blocked_requests
        self.e.enable_request(wid, rq, v)
        return int(was)


def is_free(e: SchedEnv, wid) -> bool:
    """Worker::is_free (server/worker.rs:134-137)"""
    w = e.workers[wid]
    return not w.assigned_tasks and w.mn_task is None


# ---------------------------------------------------------------------------------------------- the reference's scenarios, after their setup
def act_reject1(side, e: SchedEnv, w, t):
    """test_task_reject1: t assigned on the 4-cpu worker w.  RejectRequest(t, Some(0)): scheduling is asked for, t waits, w is free (:681-684); a tick leaves it so
    (:686-688: the pair is blocked); EnableRequest, a tick: assigned again (:703-704)"""
    assert e.task(t).is_assigned()
    rq = e.tasks[t].rq
    kinds = side.reject([(t, w, 0)])
    assert kinds == [K.HQ_REJECT_ASSIGNED] and set(kinds) & set(K.HQ_REJECT_SCHEDULES)
    assert e.task(t).is_waiting() and is_free(e, w) and e.last_reject_requeued == [(t, rq, e.tasks[t].priority)]
    assert e.workers[w].blocked_requests == {(rq, 0)}
    side.schedule()
    assert e.task(t).is_waiting() and is_free(e, w)
    assert side.enable(w, rq, 0) == 1 and not e.workers[w].blocked_requests
    assert side.enable(w, rq, 0) == 0  # (an absent pair: nothing changes)
    side.schedule()
    assert e.task(t).is_assigned() and e.task(t).worker == w


def act_reject2(side, e: SchedEnv, w, t):
    """test_task_reject2: cpus(4) | cpus(2) on a 4-cpu worker, assigned with variant 0 (:713-715); rejected with Some(0): waiting (:728); the next tick places it
    with variant 1 (:730-732) and the worker is not free (:733)"""
    x = e.task(t)
    assert x.is_assigned() and x.worker == w and x.rv == 0
    assert side.reject([(t, w, 0)]) == [K.HQ_REJECT_ASSIGNED]
    assert e.task(t).is_waiting()
    side.schedule()
    x = e.task(t)
    assert x.is_assigned() and x.worker == w and x.rv == 1 and not is_free(e, w)


def act_reject3(side, e: SchedEnv, w, t1, t2):
    """test_task_reject3: two tasks assigned on one worker, rejected in two messages: first t1 waits and t2 stays (:757-758), then both wait (:771-772)"""
    assert e.task(t1).is_assigned() and e.task(t2).is_assigned()
    assert side.reject([(t1, w, 0)]) == [K.HQ_REJECT_ASSIGNED]
    assert e.task(t1).is_waiting() and e.task(t2).is_assigned()
    assert side.reject([(t2, w, 0)]) == [K.HQ_REJECT_ASSIGNED]
    assert e.task(t1).is_waiting() and e.task(t2).is_waiting() and is_free(e, w)


def act_prefill_rejected(side, e: SchedEnv, w1, prefilled):
    """test_prefill_rejected: setup_prefill, RejectRequest(the prefilled task, Some(0)) from w1: scheduling is asked for, the task waits (:944), w1 has a blocked
    request (:945), sanity_check holds (:946: it is in no prefill set and in its queue)"""
    x = e.tasks[prefilled]
    assert x.state == core.PREFILLED
    kinds = side.reject([(prefilled, w1, 0)])
    assert kinds == [K.HQ_REJECT_PREFILLED] and set(kinds) & set(K.HQ_REJECT_SCHEDULES)
    assert x.state == core.WAITING and prefilled in e.ready[x.rq] and e.workers[w1].blocked_requests == {(x.rq, 0)}
    assert not e.workers[w1].prefilled_tasks and prefilled not in list(e.prefill.get(x.rq, (0, ()))[1])
    assert e.last_reject_requeued == [(prefilled, x.rq, x.priority)]


def act_steal_rejected(side, e: SchedEnv, w1, w2, t):
    """test_steal_rejected: setup_retracting, RejectRequest(t, Some(0)) from w1: one ComputeTasks message to w2 (:1128), no scheduling asked (emptiness_check,
    :1129), t is Assigned on w2 (:1130-1135), w1 has a blocked request (:1136)"""
    x = e.tasks[t]
    assert x.state == core.RETRACTING and x.worker == w1 and e.redirects[t][0] == w2
    v = e.redirects[t][1]
    kinds = side.reject([(t, w1, 0)])
    assert kinds == [K.HQ_REJECT_REDIRECTED] and not set(kinds) & set(K.HQ_REJECT_SCHEDULES)
    assert e.last_reject_reassigned == [(t, w2, v)] and e.last_reject_requeued == []
    assert x.state == core.ASSIGNED and x.worker == w2 and t not in e.redirects and t in e.workers[w2].assigned_tasks
    assert e.workers[w1].blocked_requests == {(x.rq, 0)}


def setup_reject1(e: SchedEnv):
    w = e.new_worker_cpus(4)
    return w, e.new_task()


def setup_reject2(e: SchedEnv):
    w = e.new_worker_cpus(4)
    return w, e.new_task(TB().cpus(4).next_variant().cpus(2))


def setup_reject3(e: SchedEnv):
    w = e.new_worker_cpus(4)
    return w, e.new_task(), e.new_task()


# ---------------------------------------------------------------------------------------------- seeded histories
FORMS = lc.FORMS
# Chosen on the CPU (tests/test_reject_oracle.py checks every condition on the mirror alone and writes profiles/reject/coverage.txt): over each form's seeds every
# accepted kind, the refused kinds _REPEAT, _WRONG_WORKER, _WRONG_VARIANT, _NONE and _RUNNING, a reject whose requeue dissolves a prefill set and an enable followed
# by a tick that places the formerly blocked request occur.
SEEDS = {"two_call": (0, 6, 9, 15), "in_tick": (2, 6, 14, 21), "view": (0, 24, 35)}
P_REJECT, P_ENABLE = 0.45, 0.35


class History(lc.History):
    """lifecycle_cases.History with ("reject", triples) and ("enable", (worker, rq, variant)) steps drawn, from the mirror's state when they are due, behind its
    own steps.  What the generator never asks for, beyond the base class's list: a reject of a Retracting task the tick has put back on the worker it is retracting
    from (no redirect was inserted for it, mapping.rs:69: the reference would make it Waiting while the worker still holds it)."""

    def __init__(self, seed: int, form: str, fixed=None):
        super().__init__(seed, form, fixed)
        self.enabled = set()  # (worker, rq, variant) pairs enabled and not yet seen placed

    def _rv(self, t, own):
        """a rejected variant: mostly `own` (the one that makes the position eligible), else None, another one of the request, or one it does not have"""
        u, nv = self.rng.random(), len(self.env.requests[t.rq])
        if u < 0.7:
            return own
        if u < 0.8:
            return NONE_V
        return int(self.rng.integers(0, nv)) if u < 0.92 else nv + int(self.rng.integers(0, 3))

    def _reporter(self, own):
        u = self.rng.random()
        return own if u < 0.82 else self._rw() if u < 0.95 else GHOST

    def _reject(self):
        e, rng, out = self.env, self.rng, []
        for x, t in sorted(e.tasks.items()):
            u = rng.random()
            if t.state == core.ASSIGNED and u < 0.3:
                out.append((x, self._reporter(t.worker), self._rv(t, t.rv)))
            elif t.state == core.RUNNING and u < 0.1:
                out.append((x, t.worker, t.rv))
            elif t.state == core.PREFILLED and u < 0.4:
                out.append((x, self._reporter(t.worker), self._rv(t, 0)))
            elif t.state == core.RETRACTING and x not in e.retaken_variant and u < 0.5:
                w = t.worker if rng.random() < 0.8 else e.redirects[x][0] if x in e.redirects else self._rw()
                out.append((x, w, self._rv(t, 0)))
            elif t.state == core.RUNNING_MN and u < 0.3:
                out.append((x, t.mn_workers[0], 0))
            elif t.state == core.WAITING and u < 0.03:
                out.append((x, self._rw(), 0))
        return ("reject", self._noise(out, lambda x: (x, self._rw(), 0)))

    def _enable(self):
        e, rng = self.env, self.rng
        pairs = sorted((wid, rq, v) for wid, w in e.workers.items() for (rq, v) in w.blocked_requests)
        if not pairs or rng.random() < 0.1:
            return ("enable", [(self._rw(), 0, 1)])  # (a pair that is most likely absent)
        k = max(1, int(len(pairs) * rng.random()))
        return ("enable", [pairs[int(j)] for j in rng.choice(len(pairs), k, replace=False)])

    def steps(self):
        for rnd, step in super().steps():
            yield rnd, step
            if self.fixed is not None:
                continue
            if self.rng.random() < P_REJECT:
                yield rnd, self._reject()
            if self.rng.random() < P_ENABLE:
                yield rnd, self._enable()


def history(seed: int, form: str, fixed=None) -> History:
    return History(seed, form, fixed)


def _apply(h: History, oracle, dev, step) -> bool:
    e, cov = h.env, h.cov
    kind, arg = step
    if kind == "reject":
        mark = len(e.retract_messages)
        n = e.reject_tasks(arg)
        for k in e.last_reject_kinds:
            cov[f"HQ_REJECT_{k}"] += 1
        if len(e.retract_messages) > mark:
            cov["reject dissolved a prefill set"] += 1
        if dev:
            dev.reject(e, arg, n)
    elif kind == "enable":
        mark = len(e.retract_messages)
        for (wid, rq, v) in arg:
            if wid not in e.workers:
                continue
            was = (rq, v) in e.workers[wid].blocked_requests
            e.enable_request(wid, rq, v)
            if was:
                h.enabled.add((wid, rq, v)); cov["enable"] += 1
            if dev:
                dev.enable(e, wid, rq, v, was)
    else:
        held = {x for x, t in e.tasks.items() if t.state == core.ASSIGNED} if kind == "tick" else None
        ok = lc._apply(h, oracle, dev, step)
        if kind == "tick" and ok:
            for x, t in e.tasks.items():
                if t.state == core.ASSIGNED and x not in held and (t.worker, t.rq, t.rv) in h.enabled:
                    h.enabled.discard((t.worker, t.rq, t.rv)); cov["tick placed an enabled request"] += 1
        return ok
    lc._disposed(h, dev, mark)
    if dev:
        dev.check(e)
    return True


def play(h: History, oracle, dev=None) -> History:
    """lifecycle_cases.play with the two new steps"""
    h.deps_given, h.inserts = {}, 0
    try:
        if dev:
            dev.seed(h.env)
        for rnd, step in h.steps():
            h.log.append((rnd, step))
            if not _apply(h, oracle, dev, step):
                h.ended_early = rnd
                break
        if dev:
            dev.end(h.env)
    except Exception as err:
        raise AssertionError(f"{type(err).__name__}: {err}\n{h.describe()}") from err
    return h


def coverage_lines(cov_by_form) -> list:
    """the coverage table of profiles/reject/coverage.txt: one line per counter, a column per form"""
    keys = sorted({k for c in cov_by_form.values() for k in c if k.startswith("HQ_REJECT_") or k in ("reject dissolved a prefill set", "enable", "tick placed an enabled request")},
                  key=lambda k: (not k.startswith("HQ_REJECT_"), int(k.rsplit("_", 1)[1]) if k.startswith("HQ_REJECT_") else 0, k))
    names = {getattr(abi, n): n for n in dir(abi) if n.startswith("HQ_REJECT_") and isinstance(getattr(abi, n), int)}
    lines = [f"{'counter':<34}" + "".join(f"{f:>10}" for f in FORMS)]
    for k in keys:
        label = names[int(k.rsplit("_", 1)[1])] if k.startswith("HQ_REJECT_") else k
        lines.append(f"{label:<34}" + "".join(f"{cov_by_form[f].get(k, 0):>10}" for f in FORMS))
    return lines
