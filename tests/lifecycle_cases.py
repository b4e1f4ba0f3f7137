"""Seeded histories of whole task lifecycles on one resident state: ticks (two calls, with another call or an abandoning delta between them, or consumed inside the
tick), start / finish / fail / cancel batches, retract responses, workers lost and added, new tasks -- interleaved on ONE SchedEnv, which is the mirror pinned to
the reference by the test_*_oracle.py files.  history(seed, form) draws the steps from the mirror's state as it stands when a step is due; play() applies them to
the mirror and, through a device side (tests/resident_checks.py: DeviceSide), to a context.  tests/test_lifecycle_oracle.py plays every history on the mirror alone,
with the CPU oracle as the scheduler; tests/test_gpu_lifecycle.py plays the same histories on the device.  Also the deterministic scenario of a two-call tick that
selects nothing and redirects a prefilled task.  Not a test module.

What the generator never asks for, and why (each a state no worker or host produces):
  * a prefilled or Retracting task reported Running by a worker that holds a multi-node task (that worker starts nothing else), or by one that has no room for
    the variant it names (a worker starts what fits).  free.remove saturates there (workerload.rs:156-165) and the later releases leave free > total: a state
    the reference's Worker::sanity_check asserts on, and from which its next tick places a multi-node task on a worker it also gives single-node tasks
    (a worker of 6 cpus with a free amount of 9: the oracle put a 2-node task and two single-node tasks on it).  The single-call tests keep the over-committed rows (test_order_under_saturation and its kin);
  * a retract response for a Retracting task the tick has put back on the worker it is retracting from (mapping.rs:69 inserts no redirect: the reference keeps
    no record the response could resolve);
  * losing a worker that holds a prefilled task together with an assigned task of a higher priority than that prefill set: on_remove_worker requeues the
    assigned task first, add_ready_task dissolves the set (taskqueue.rs:146-152), and move_prefilled_task_to_ready then unwraps the set that is gone
    (taskqueue.rs:264): the reference panics; nor one that holds a Retracting task the tick has put back on it: no redirect was inserted for it
    (mapping.rs:69) and reactor.rs:91 asserts that there is one;
  * a task that has dependencies and a user priority: a consumer that a finish batch releases would dissolve the lower-priority prefill sets in the middle of the
    batch (add_ready_task), which the reference, taking one message at a time, follows with process_retracted before the next message -- a step that is the
    host's (hqtick_assigned_unprefill + hqtick_retracting_add) and cannot happen inside one hqtick_finish_tasks call.  Arrivals and lost workers dissolve them;
  * losing a worker when two or fewer are left."""
from __future__ import annotations

import collections
import re

import numpy as np

from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

CFG = dict(time_limit_s=20.0)
FORMS = ("two_call", "in_tick", "view")
# Chosen on the CPU (tests/test_lifecycle_oracle.py checks every condition): each history completes at least four rounds, at most a quarter of a form's seeds ends
# early -- at a tick the reference itself refuses -- no history places a multi-node task on a worker that still holds prefilled tasks (out of scope by design,
# DESIGN.md §8g), and over each form's seeds every kind of answer and event occurs in at least two of them.  The last seeds below 1000 of each form are ones that
# end early; seed 1000 is the form's long history (60 cheap rounds), which enters more entries than the ledger's first table holds before it is rebuilt.
SEEDS = {"two_call": (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 13, 14, 15, 17, 18, 19, 20, 21, 22, 23, 27, 45, 50, 72, 61, 101, 1000),
         "in_tick": (1, 3, 4, 5, 6, 7, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19, 22, 23, 24, 26, 27, 59, 64, 65, 47, 1000),
         "view": (2, 3, 8, 9, 15, 17, 34, 116, 121, 0, 89, 1000)}
UNKNOWN = 10**12
LONG_FROM = 1000
NO = abi.HQ_NO_WORKER
LIVE_HELD = (core.ASSIGNED, core.RUNNING)


def _shapes(gpu):
    # (a two-variant request, one with the named resource, cpus_all so that ALL entries meet AMOUNT entries, a 2-node request)
    return [TB().cpus(1), TB().cpus(2), TB().cpus(3).next_variant().cpus(1), TB().cpus(1).add_resource(gpu, 1), TB().cpus(2).next_variant().cpus(1).add_resource(gpu, 1),
            TB().cpus_all(), TB().n_nodes(2)]


SHAPE_P = np.array([0.3, 0.18, 0.16, 0.1, 0.1, 0.08, 0.08])


class History:
    def __init__(self, seed: int, form: str, fixed=None):
        assert form in FORMS
        self.seed, self.form = seed, form
        self.long = seed >= LONG_FROM
        self.rng = rng = np.random.default_rng([seed, FORMS.index(form), 77])
        self.lean = bool(rng.random() < 0.4)        # few tasks, few arrivals: the ready set runs empty and ticks live off the prefill sets
        self.env = e = SchedEnv(abi.make_config(reserve=1, fill_max=2, **CFG))
        gpu = e.new_named_resource("gpus")
        self.shapes = _shapes(gpu)
        for s in self.shapes:
            e.rq_id(s)
        for _ in range(int(rng.integers(3, 7))):
            e.new_worker(WB(int(rng.integers(2, 7))).res_sum("gpus", 2))
        n = int(rng.integers(40, 51)) if self.lean else int(rng.integers(55, 81))
        n_roots = n * 3 // 5
        for k in range(n):
            deps = [] if k < n_roots else self._deps(sorted(e.tasks), int(rng.integers(1, 3)))
            e.new_task(self._builder(self._shape(), 0 if deps else self._prio(), deps))
        # seeds from LONG_FROM on: many cheap rounds (a dozen arrivals, nearly everything started and finished each round) that pile up more entries and
        # tombstones than the ledger's first table holds -- the claim words and running bytes cross a rebuild in the middle of everything else
        self.n_rounds = 60 if self.long else int(rng.integers(5, 9))
        self.fixed = fixed  # an explicit step list instead of drawn steps (a minimised finding)
        self.log, self.cov, self.rounds_done, self.ended_early = [], collections.Counter(), 0, None

    # ---- draws
    def _shape(self):
        k = int(self.rng.choice(len(self.shapes), p=SHAPE_P))
        return 0 if self.long and k == 6 and self.rng.random() < 0.7 else k  # (a long history draws fewer 2-node tasks: they idle its few workers)

    def _prio(self):
        return 0 if self.rng.random() < 0.85 else int(self.rng.integers(1, 3))

    def _deps(self, pool, k):
        return [pool[int(j)] for j in self.rng.choice(len(pool), min(k, len(pool)), replace=False)]

    def _builder(self, shape, prio, deps):
        b = self.shapes[shape]
        if prio:
            b = b.user_priority(prio)
        return b.task_deps(deps) if deps else b

    def _rw(self):
        wids = sorted(self.env.workers)
        return wids[int(self.rng.integers(0, len(wids)))]

    def _variant(self, t):
        nv = len(self.env.requests[t.rq])
        return int(self.rng.integers(0, nv)) if self.rng.random() < 0.88 else nv + int(self.rng.integers(0, 4))

    def _noise(self, batch, unknown):
        rng = self.rng
        if batch:
            batch = batch + [batch[int(rng.integers(0, len(batch)))] for _ in range(max(1, len(batch) // 5))]
        batch = batch + [unknown(UNKNOWN + int(rng.integers(0, 50))) for _ in range(2)]
        return [batch[int(k)] for k in rng.permutation(len(batch))]

    # ---- the batches, from the mirror's state now
    def _fits(self, room, wid, rq, v) -> bool:
        """variant v of request rq fits worker wid's free row in `room` (ALL: the whole resource is free); if so it is taken from there"""
        e = self.env
        if not 0 <= v < len(e.requests[rq]):
            return True  # (refused as a bad variant: takes nothing)
        w = e.workers[wid]
        free = room.setdefault(wid, list(w.free) + [0] * (e.n_resources - len(w.free)))
        total = list(w.total) + [0] * (e.n_resources - len(w.total))
        ent = e.requests[rq][v]["entries"]
        if not all(free[r] >= a if kind == abi.HQ_ENTRY_AMOUNT else (free[r] == total[r] and total[r] > 0) for (r, kind, a) in ent):
            return False
        for (r, kind, a) in ent:
            free[r] = free[r] - a if kind == abi.HQ_ENTRY_AMOUNT else 0
        return True

    def _start(self):
        e, rng, out, room = self.env, self.rng, [], {}
        for x, t in sorted(e.tasks.items()):
            u = rng.random()
            if t.state == core.ASSIGNED and u < 0.5:
                out.append((x, t.worker if rng.random() < 0.85 else self._rw(), t.rv if rng.random() < 0.85 else int(rng.integers(0, 3))))
            elif t.state == core.RUNNING and u < 0.15:
                out.append((x, t.worker, t.rv if rng.random() < 0.6 else int(rng.integers(0, 3))))
            elif t.state in (core.PREFILLED, core.RETRACTING) and u < 0.45 and e.workers[t.worker].sn():
                w, v = t.worker, self._variant(t)
                if rng.random() > 0.8:
                    w = e.redirects[x][0] if t.state == core.RETRACTING and x in e.redirects else self._rw()
                if w != t.worker or self._fits(room, w, t.rq, v):
                    out.append((x, w, v))
            elif t.state == core.RUNNING_MN and u < 0.5:
                ws = t.mn_workers
                out.append((x, ws[0] if rng.random() < 0.7 or len(ws) < 2 else ws[1], 0))
            elif t.state == core.WAITING and u < 0.03:
                out.append((x, self._rw(), 0))
        return ("start", self._noise(out, lambda x: (x, self._rw(), 0)))

    def _reported(self, p_held, p_retr, p_pf, p_mn):
        """(id, reporter) pairs as test_twin_contexts_on_a_random_history draws them, with multi-node tasks by root and by non-root"""
        e, rng, out = self.env, self.rng, []
        for x, t in sorted(e.tasks.items()):
            u = rng.random()
            if t.state in LIVE_HELD and u < p_held:
                out.append((x, t.worker if rng.random() < 0.85 else self._rw()))
            elif t.state == core.RETRACTING and u < p_retr:
                out.append((x, t.worker if rng.random() < 0.7 or x not in e.redirects else e.redirects[x][0]))
            elif t.state == core.PREFILLED and u < p_pf:
                out.append((x, t.worker if rng.random() < 0.85 else self._rw()))
            elif t.state == core.RUNNING_MN and u < p_mn:
                ws = t.mn_workers
                out.append((x, ws[0] if rng.random() < 0.7 or len(ws) < 2 else ws[1]))
        return out

    def _finish(self):
        e, rng = self.env, self.rng
        out = self._reported(0.55, 0.5, 0.25, 0.5)
        out += [(x, self._rw()) for x, t in sorted(e.tasks.items()) if t.state == core.WAITING and rng.random() < 0.02]
        return ("finish", self._noise(out, lambda x: (x, self._rw())))

    def _fail(self):
        e, rng = self.env, self.rng
        out = self._reported(0.12, 0.25, 0.25, 0.25)
        for x, w in list(out):  # a consumer of a producer of the batch, reported as a waiting task: accepted before the producer, gone after it
            cons = [c for c in e.tasks[x].consumers if e.tasks[c].state == core.WAITING]
            if cons and rng.random() < 0.5:
                out.append((cons[int(rng.integers(0, len(cons)))], NO))
        for x, t in sorted(e.tasks.items()):
            u = rng.random()
            if t.state == core.WAITING and u < 0.05:
                out.append((x, NO if rng.random() < 0.6 else self._rw()))
            elif t.state in LIVE_HELD + (core.PREFILLED, core.RETRACTING, core.RUNNING_MN) and u < 0.04:
                out.append((x, NO))
        return ("fail", self._noise(out, lambda x: (x, NO if rng.random() < 0.5 else self._rw())))

    def _cancel(self):
        e, rng = self.env, self.rng
        p = {core.WAITING: 0.05, core.ASSIGNED: 0.1, core.RUNNING: 0.1, core.PREFILLED: 0.2, core.RETRACTING: 0.2, core.RUNNING_MN: 0.25, core.FINISHED: 0.04}
        out = [x for x, t in sorted(e.tasks.items()) if rng.random() < p[t.state]]
        return ("cancel", self._noise(out, lambda x: x))

    def _retract(self):
        e, rng, by = self.env, self.rng, {}
        for x, t in sorted(e.tasks.items()):
            if t.state == core.RETRACTING and x not in e.retaken_variant and rng.random() < 0.75:
                by.setdefault(t.worker, []).append(x)
        out = [(w, [ids[int(k)] for k in rng.permutation(len(ids))] + [UNKNOWN]) for w, ids in sorted(by.items())]
        return ("retract", out)

    def _lose(self):
        e, rng = self.env, self.rng
        if len(e.workers) <= 2:
            return None
        score = {}
        for wid, w in e.workers.items():
            s = 1.0 + 2.0 * len(w.prefilled_tasks) + (3.0 if not w.sn() else 0.0)
            s += sum(1.0 if e.tasks[x].state == core.RUNNING else 0.3 for x in w.assigned_tasks)
            score[wid] = s
        for x, t in e.tasks.items():
            if t.state == core.RETRACTING:
                score[t.worker] = score.get(t.worker, 0) + 3.0
                if x in e.redirects:
                    score[e.redirects[x][0]] += 3.0
        for wid, w in e.workers.items():  # (the reference panics on these: the module's docstring)
            if any(x in e.retaken_variant for x in w.assigned_tasks):
                del score[wid]
                continue
            if w.sn() and w.prefilled_tasks and w.assigned_tasks:
                low = min(e.prefill[e.tasks[x].rq][0] for x in w.prefilled_tasks)
                if max(e.tasks[x].priority for x in w.assigned_tasks) > low:
                    del score[wid]
        wids = sorted(score)
        if not wids:
            return None
        pr = np.array([score[w] for w in wids]); pr = pr / pr.sum()
        return ("lose", wids[int(rng.choice(len(wids), p=pr))])

    def _add_worker(self):
        return ("add_worker", int(self.rng.integers(2, 7)))

    def _new_tasks(self, n=None, free=False):
        """specs (shape, user priority, deps): some depend on unfinished tasks, some on finished ones, some on earlier tasks of the batch; free: none has a dependency"""
        e, rng = self.env, self.rng
        n = n or (int(rng.integers(2, 6)) if self.lean else int(rng.integers(5, 14)))
        live = [x for x, t in sorted(e.tasks.items()) if t.state != core.FINISHED]
        done = [x for x, t in sorted(e.tasks.items()) if t.state == core.FINISHED]
        specs = []
        for k in range(n):
            deps, u = [], rng.random()
            if not free and u < 0.3 and live:
                deps += self._deps(live, int(rng.integers(1, 3)))
            if not free and 0.2 < u < 0.45 and done:
                deps += self._deps(done, 1)
            if not free and u > 0.85 and k:
                deps.append(("new", int(rng.integers(0, k))))
            specs.append((self._shape(), 0 if deps else self._prio(), deps))
        return ("new_tasks", specs)

    def _tick(self):
        between, u = None, self.rng.random()
        if self.form != "in_tick":
            if u < 0.25:
                which = ("start", "finish", "fail", "cancel", "lose", "add_worker")[int(self.rng.integers(0, 6))]
                between = ("refused", "retract" if which == "add_worker" and (self.seed + len(self.log)) % 2 else which)
            elif u < 0.42:
                between = ("abandon", self._new_tasks(n=int(self.rng.integers(1, 4)), free=True)[1])
        return ("tick", between)

    def steps(self):
        """(round, step), each drawn when it is due"""
        rng, e = self.rng, self.env
        if self.fixed is not None:
            rnd = -1
            for step in self.fixed:
                rnd += step[0] == "tick"
                yield rnd, step
                self.rounds_done = rnd + 1
            return
        events = [self._start, self._finish, self._fail, self._cancel, self._retract, self._lose, self._add_worker, self._new_tasks]
        p = np.array([0.22, 0.22, 0.08, 0.08, 0.14, 0.08, 0.08, 0.1])
        if self.lean:
            p = np.array([0.24, 0.3, 0.06, 0.06, 0.14, 0.08, 0.08, 0.04])
        p = p / p.sum()
        drains = 0
        for rnd in range(self.n_rounds):
            yield rnd, self._tick()
            if self.long:
                yield rnd, self._new_tasks(n=int(rng.integers(14, 22)))
                yield rnd, self._start()
                yield rnd, ("finish", self._noise(self._reported(0.95, 0.6, 0.1, 0.9), lambda x: (x, self._rw())))
            for _ in range(1 if self.long else int(rng.integers(1, 4))):
                for k in rng.choice(len(events), int(rng.integers(2, 5)), replace=False, p=p):
                    step = events[int(k)]()
                    if step is not None:
                        yield rnd, step
            if self.long or rng.random() < 0.6:  # most retracts are answered before the next tick: one that meets a Retracting task where it would prefill is refused
                yield rnd, self._retract()
            if self.lean and drains < 2 and rng.random() < 0.5 and any(t.state == core.PREFILLED for t in e.tasks.values()):
                # whatever is ready is cancelled while tasks are prefilled on busy workers, and a worker with room joins: the next tick can only redirect
                drains += 1
                ready = sorted(x for s in e.ready.values() for x in s)
                if ready:
                    yield rnd, ("cancel", ready)
                yield rnd, ("add_worker", 6)
            self.rounds_done = rnd + 1

    def describe(self) -> str:
        lines = [f"lifecycle history seed={self.seed} form={self.form} lean={self.lean}: failed at round {self.log[-1][0] if self.log else '-'}, step {len(self.log) - 1}; the steps so far:"]
        lines += [f"  [{k}] round {rnd}: {step!r}" for k, (rnd, step) in enumerate(self.log)]
        return "\n".join(lines)


def history(seed: int, form: str, fixed=None) -> History:
    return History(seed, form, fixed)


# ---------------------------------------------------------------------------------------------- the driver
def oracle_tick(oracle, snap):
    """-> (result, status); a tick the reference refuses: (None, its negative code)"""
    try:
        res = oracle.tick(snap)
        return res, res.status
    except RuntimeError as err:
        m = re.search(r"failed: (-\d+)", str(err))
        assert m, err
        return None, int(m.group(1))


def enters_something(e: SchedEnv, res) -> bool:
    """the tick's result has something that becomes state at the consume"""
    R = e.n_resources
    free = np.array([list(e.workers[w].free) + [0] * (R - len(e.workers[w].free)) for w in sorted(e.workers)], np.uint64).reshape(len(e.workers), R)
    sn = np.array([e.workers[w].sn() for w in sorted(e.workers)], bool)
    return bool(any(res.records) or res.redirects or res.mn or (np.asarray(res.new_free, np.uint64)[sn] != free[sn]).any())


def _disposed(h, dev, mark):
    """process_retracted outside a tick (server/reactor.rs:34-62) is the host's: the prefill sets a higher-priority arrival dissolved"""
    e = h.env
    msgs = e.retract_messages[mark:]
    if msgs:
        h.cov["disposed prefill set"] += 1
        if dev:
            dev.disposed(e, msgs)
    return len(e.retract_messages)


def _new_tasks(h, specs):
    e, ids = h.env, []
    for shape, prio, deps in specs:
        deps = sorted({ids[d[1]] if isinstance(d, tuple) else d for d in deps})
        ids.append(e.new_task(h._builder(shape, prio, deps)))
        h.deps_given[ids[-1]] = deps
    return ids


def _apply(h: History, oracle, dev, step) -> bool:
    e, cov = h.env, h.cov
    kind, arg = step
    mark = len(e.retract_messages)
    if kind == "tick":
        snap = e.snapshot()
        want, code = oracle_tick(oracle, snap)
        if dev:
            want = dev.tick(e, snap, want, code)
        if code < 0:
            cov[f"tick refused {code}"] += 1
            return False
        two_call = h.form != "in_tick"
        pend = enters_something(e, want)
        abandoned = False
        if arg is not None and two_call:
            if arg[0] == "refused":
                if pend:
                    cov["refused while pending"] += 1
                    if dev:
                        dev.refused(e, arg[1])
            else:
                ids = _new_tasks(h, arg[1])
                if dev:
                    dev.new_tasks(e, ids, h.deps_given)
                abandoned = True
                cov["abandoned two-call tick"] += 1
                if want.redirects or any(want.retracts):
                    cov["abandoned tick with retracts"] += 1
        if not abandoned:
            if dev and two_call:
                dev.consume(e, want)
            e.apply(want)
            recs = [r for rs in want.records for r in rs]
            for (_, _, k) in recs:
                cov["PREFILL record" if k == abi.HQ_REC_PREFILL else "ASSIGN record"] += 1
            h.inserts += len(recs) + len(want.redirects) + len(want.mn)
            for k in want.redirect_kinds:
                cov[("HQ_REDIRECT_FROM_PREFILL", "HQ_REDIRECT_RETARGET", "HQ_REDIRECT_SAME_WORKER")[k]] += 1
            cov["retract"] += sum(len(r) for r in want.retracts)
            cov["multi-node placement"] += len(want.mn)
            wids = sorted(e.workers)
            cov["multi-node placement on a worker with prefilled tasks"] += sum(1 for (_, ws) in want.mn for k in ws if e.workers[wids[k]].prefilled_tasks)
            if not recs and not want.mn and want.redirects and all(k == abi.HQ_REDIRECT_FROM_PREFILL for k in want.redirect_kinds):
                cov["two-call tick, zero selected, a redirect" if two_call else "in-tick tick, zero selected, a redirect"] += 1
    elif kind == "start":
        n = e.start_tasks(arg)
        for k in e.last_start_kinds:
            cov[f"HQ_START_{k}"] += 1
        if dev:
            dev.start(e, arg, n)
    elif kind == "finish":
        rel = e.finish_tasks(arg)
        for k in e.last_finish_kinds:
            cov[f"HQ_FINISH_{k}"] += 1
        if dev:
            dev.finish(e, arg, rel)
    elif kind == "fail":
        n = e.fail_tasks(arg)
        for k in e.last_fail_kinds:
            cov[f"HQ_FAIL_{k}"] += 1
        if dev:
            dev.fail(e, arg, n)
    elif kind == "cancel":
        before = {x for x, t in e.tasks.items() if t.state != core.FINISHED}
        msgs = e.cancel_tasks(arg)
        for (_, k) in e.last_cancel_routes:
            cov[f"HQ_CANCEL_{k}"] += 1
        if dev:
            dev.cancel(e, arg, msgs, sorted(before - {x for x, t in e.tasks.items() if t.state != core.FINISHED}))
    elif kind == "retract":
        for wid, ids in arg:
            if wid not in e.workers:
                continue
            want = [(x, *e.redirects[x]) for x in ids if x in e.tasks and e.tasks[x].state == core.RETRACTING and e.tasks[x].worker == wid and x in e.redirects]
            n_left = sum(1 for x in ids if x in e.tasks and e.tasks[x].state == core.RETRACTING and e.tasks[x].worker == wid)
            e.retract_response(wid, [x for x in ids if x in e.tasks])  # (an id nobody knows reaches the library only: it is ignored there)
            cov["retract response"] += n_left
            if dev:
                dev.retract(e, wid, ids, want, n_left)
    elif kind == "lose":
        w = e.workers[arg]
        held = set(w.assigned_tasks)
        if any(e.tasks[x].state == core.RUNNING for x in held):
            cov["lost worker with a running task"] += 1
        if w.sn() and w.prefilled_tasks:
            cov["lost worker with a prefilled task"] += 1
        if any(t.state == core.RETRACTING and t.worker == arg for t in e.tasks.values()):
            cov["lost worker with a Retracting task"] += 1; cov["  (retracting from it)"] += 1
        if any(e.tasks[x].state == core.RETRACTING for x in held):
            cov["lost worker with a Retracting task"] += 1; cov["  (a redirect's target)"] += 1
        if not w.sn():
            cov["lost worker with a multi-node task"] += 1
        info = dict(ready_before={x for s in e.ready.values() for x in s}, prefilled=sorted(w.prefilled_tasks) if w.sn() else [])
        info["sent"] = e.remove_worker(arg)
        info["disposed"] = [x for (_, x) in e.retract_messages[mark:]]  # (back in their queues in the mirror already; the host's part comes after the call)
        if dev:
            dev.lose(e, arg, info)
    elif kind == "add_worker":
        wid = e.new_worker(WB(arg).res_sum("gpus", 2))
        if dev:
            dev.add_worker(e, wid)
    elif kind == "new_tasks":
        ids = _new_tasks(h, arg)
        if dev:
            dev.new_tasks(e, ids, h.deps_given)
    else:
        raise AssertionError(kind)
    _disposed(h, dev, mark)
    if dev:
        dev.check(e)
    return True


def play(h: History, oracle, dev=None) -> History:
    """the history on its mirror and, with dev, on a context; an assertion that fails anywhere names the seed, the form, the round and the steps so far"""
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


# ---------------------------------------------------------------------------------------------- the zero-selection two-call tick
def zero_selection_env(tick, on_cancel=None, on_add_worker=None):
    """prefilled tasks and an empty ready set, then a worker with room: test_reactor.rs:775-795's setup (reserve 1, one prefilled task at most; three tasks on one
    1-cpu worker: one assigned, one prefilled, one waiting), the waiting task cancelled, a second 1-cpu worker joins.  The next tick can only take the prefilled
    task for the new worker: a retract on w1, a FROM_PREFILL redirect to w2, no record.  tick(e, snap) -> the first tick's result; on_cancel(e, ids) and
    on_add_worker(e, wid) tell a context.  -> (mirror, w1, w2, the assigned task, the prefilled task)"""
    e = SchedEnv(abi.make_config(reserve=1, fill_max=1, **CFG))
    tasks = e.new_tasks(3, TB())
    w1 = e.new_worker(WB(1))
    e.apply(tick(e, e.snapshot()))
    assigned = next(t for t in tasks if e.task(t).is_assigned()); prefilled = next(t for t in tasks if e.task(t).is_prefilled())
    (waiting,) = [t for t in tasks if e.task(t).is_waiting()]
    assert e.cancel_tasks([waiting]) == {}
    if on_cancel:
        on_cancel(e, [waiting])
    w2 = e.new_worker(WB(1))
    if on_add_worker:
        on_add_worker(e, w2)
    assert not any(e.ready.values())
    return e, w1, w2, assigned, prefilled


def check_zero_selection_result(e, res, w1, w2, prefilled):
    wids = sorted(e.workers)
    assert res.status >= 0 and not any(res.records) and not res.mn
    assert res.retracts == [[prefilled] if w == w1 else [] for w in wids]
    assert res.redirects == [(prefilled, wids.index(w2), 0)] and res.redirect_kinds == [abi.HQ_REDIRECT_FROM_PREFILL]
    assert res.new_free.tolist() == [[0], [0]]
