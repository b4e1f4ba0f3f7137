"""Lost workers in batches on SchedEnv, shared by tests/test_lose_oracle.py (the mirror alone, the CPU oracle as the scheduler) and tests/test_gpu_lose.py (the
same through hqtick_lose_workers).  Seeded histories: lifecycle_cases.History whose loss events take 1 to 4 workers at once -- a first worker drawn by the base
class's weights, then, more often than chance would, the workers that make a batch interesting: another member of its multi-node task, the other end of a
Retracting task's redirect -- in ascending, descending or shuffled order.  A few more workers join at the start, so that batches of four fit.

The generator keeps the base class's exclusions (tests/lifecycle_cases.py's docstring), now for the batch as a whole:
  * no lost worker holds a Retracting task the tick has put back on it;
  * no task the batch requeues with add_ready_task (assigned, running, a redirect's entry, a multi-node task by its root) has a higher priority than the prefill
    set of a prefilled task on ANY worker of the batch: one call per worker, as the reference's handler takes them, would dissolve that set in the middle;
  * never a batch after which two or fewer workers would be left.
Not a test module."""
from __future__ import annotations

import numpy as np

import lifecycle_cases as lc
from hyperqueue_amd import abi, core
from hyperqueue_amd.core import SchedEnv, WorkerBuilder as WB

K = abi
FORMS = lc.FORMS
# Chosen on the CPU (tests/test_lose_oracle.py checks every line of LINES on the mirror alone and writes profiles/lose/coverage.txt): over all seeds together every
# line is reached at least once.
SEEDS = {"two_call": (2, 8, 9), "in_tick": (0, 13), "view": (1, 2)}
KIND_NAMES = ("HQ_LOSE_ASSIGNED", "HQ_LOSE_RUNNING", "HQ_LOSE_PREFILLED", "HQ_LOSE_MN_ROOT", "HQ_LOSE_REDIRECT")
LINES = KIND_NAMES + ("a non-root member listed", "root and non-root of one task in one batch", "old and redirect target of one Retracting task in one batch",
                      "old alone with a redirect (reassigned)", "a worker with no entry at all", "a batch in descending row order")
MORE = ("lose batch", "lost workers", "batch of 1", "batch of 2", "batch of 3", "batch of 4", "lose dissolved a prefill set")


class History(lc.History):
    """lifecycle_cases.History with ("lose", [worker ids]) steps of 1 to 4 workers"""

    def __init__(self, seed: int, form: str, fixed=None):
        super().__init__(seed, form, fixed)
        extra = np.random.default_rng([seed, lc.FORMS.index(form), 78])  # (its own stream: the base class's draws stay what they are)
        for _ in range(int(extra.integers(2, 5))):
            self.env.new_worker(WB(int(extra.integers(2, 7))).res_sum("gpus", 2))

    def _allowed(self, batch) -> bool:
        e = self.env
        if len(e.workers) - len(batch) <= 2:
            return False
        low, high = None, None
        for wid in batch:
            w = e.workers[wid]
            if any(x in e.retaken_variant for x in w.assigned_tasks):
                return False
            if w.sn():
                for x in w.prefilled_tasks:
                    p = e.prefill[e.tasks[x].rq][0]
                    low = p if low is None else min(low, p)
                held = list(w.assigned_tasks)
            else:
                tid = w.mn_task[0]
                held = [tid] if e.tasks[tid].mn_workers[0] == wid else []
            for x in held:
                p = e.tasks[x].priority
                high = p if high is None else max(high, p)
        return low is None or high is None or high <= low

    def _partners(self, wid):
        """the workers that share something with wid: the members of its multi-node task, the other end of a redirect"""
        e, out = self.env, []
        w = e.workers[wid]
        if not w.sn():
            out += [x for x in e.tasks[w.mn_task[0]].mn_workers if x != wid and x in e.workers]
        for x, t in sorted(e.tasks.items()):
            if t.state == core.RETRACTING and x in e.redirects:
                if t.worker == wid and e.redirects[x][0] in e.workers:
                    out.append(e.redirects[x][0])
                elif e.redirects[x][0] == wid and t.worker in e.workers:
                    out.append(t.worker)
        return out

    def _lose(self):
        e, rng = self.env, self.rng
        first = super()._lose()
        if first is None:
            return None
        batch = [first[1]]
        want = int(rng.choice([1, 2, 3, 4], p=[0.3, 0.3, 0.25, 0.15]))
        while len(batch) < want:
            partners = [x for w in batch for x in self._partners(w) if x not in batch]
            rest = [x for x in sorted(e.workers) if x not in batch]
            if not rest:
                break
            idle = [x for x in rest if e.workers[x].sn() and not e.workers[x].assigned_tasks and not e.workers[x].prefilled_tasks]
            u = rng.random()
            cand = partners[int(rng.integers(0, len(partners)))] if partners and u < 0.6 else idle[int(rng.integers(0, len(idle)))] if idle and u < 0.75 else rest[int(rng.integers(0, len(rest)))]
            if not self._allowed(batch + [cand]):
                break
            batch.append(cand)
        if not self._allowed(batch):
            return None
        u = rng.random()
        batch = sorted(batch) if u < 0.35 else sorted(batch, reverse=True) if u < 0.7 else [batch[int(k)] for k in rng.permutation(len(batch))]
        return ("lose", batch)


def history(seed: int, form: str, fixed=None) -> History:
    return History(seed, form, fixed)


def expected_running(e: SchedEnv) -> list:
    """on_remove_worker's running_tasks per lost worker, from the kinds of the mirror's last lose_workers"""
    return [[x[0] for x in rows if x[3] in K.HQ_LOSE_RUNNING_TASKS] for rows in e.last_lose_per_worker]


def _apply(h: History, oracle, dev, step) -> bool:
    e, cov = h.env, h.cov
    kind, arg = step
    if kind != "lose":
        return lc._apply(h, oracle, dev, step)
    mark = len(e.retract_messages)
    lost = set(arg)
    for x, t in e.tasks.items():
        if t.state == core.RUNNING_MN and t.mn_workers[0] in lost and lost & set(t.mn_workers[1:]):
            cov["root and non-root of one task in one batch"] += 1
        if t.state == core.RETRACTING and t.worker in lost and x in e.redirects and e.redirects[x][0] in lost:
            cov["old and redirect target of one Retracting task in one batch"] += 1
    info = dict(ready_before={x for s in e.ready.values() for x in s}, member={w for w in arg if not e.workers[w].sn()})
    info["n"] = e.lose_workers(arg)
    info["disposed"] = [x for (_, x) in e.retract_messages[mark:]]  # (back in their queues in the mirror already; the host's part comes after the call)
    cov["lose batch"] += 1; cov["lost workers"] += len(arg); cov[f"batch of {len(arg)}"] += 1
    for wid, rows in zip(arg, e.last_lose_per_worker):
        for x in rows:
            cov[KIND_NAMES[x[3]]] += 1
        if not rows and wid not in info["member"]:
            cov["a worker with no entry at all"] += 1
    cov["a non-root member listed"] += len(e.last_lose_mn_left)
    cov["old alone with a redirect (reassigned)"] += len(e.last_lose_reassigned)
    if len(arg) > 1 and list(arg) == sorted(arg, reverse=True):
        cov["a batch in descending row order"] += 1
    if info["disposed"]:
        cov["lose dissolved a prefill set"] += 1
    if dev:
        dev.lose(e, arg, info)
    lc._disposed(h, dev, mark)
    if dev:
        dev.check(e)
    return True


def play(h: History, oracle, dev=None) -> History:
    """lifecycle_cases.play with the batched loss"""
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
    """the coverage table of profiles/lose/coverage.txt: one line per counter, a column per form and their sum"""
    lines = [f"{'counter':<62}" + "".join(f"{f:>10}" for f in FORMS) + f"{'all':>10}"]
    for k in LINES + MORE:
        row = [cov_by_form[f].get(k, 0) for f in FORMS]
        lines.append(f"{k:<62}" + "".join(f"{v:>10}" for v in row) + f"{sum(row):>10}")
    return lines


def mirror_state(e: SchedEnv) -> dict:
    """everything of the mirror a lost worker can change, in a form that compares with =="""
    return dict(
        tasks={x: (t.state, t.worker, t.rv, None if t.mn_workers is None else list(t.mn_workers)) for x, t in e.tasks.items()},
        workers={w: (list(x.free), sorted(x.assigned_tasks), sorted(x.prefilled_tasks), sorted(x.blocked_requests), x.mn_task) for w, x in e.workers.items()},
        worker_order=list(e.worker_map), ready={q: sorted(s) for q, s in e.ready.items()}, prefill={q: (p, sorted(s)) for q, (p, s) in e.prefill.items()},
        redirects=dict(e.redirects), retaken=dict(e.retaken_variant), messages=list(e.retract_messages))
