"""Whole task lifecycles on ONE context: the seeded histories of tests/lifecycle_cases.py -- ticks in the two-call form (with a call that must be refused as
pending, or a delta that abandons the tick, between the two calls), consumed inside the tick, and on the ordered view; start / finish / fail / cancel batches,
retract responses, workers lost and added, new tasks, interleaved -- with the call's own answer, every tick against the CPU oracle on the mirror's snapshot, the
whole resident state and the audit (CROSS and STRICT) compared with the SchedEnv mirror after every step (tests/resident_checks.py).  tests/test_lifecycle_oracle.py
holds the coverage conditions of these seeds.  And the regression of the two-call tick that selects nothing but redirects a prefilled task: its placement used to
be dropped between the two calls."""
import os
import subprocess
import sys

import pytest

import cancel_cases as cc
import lifecycle_cases as lc
import resident_checks as rc
import test_gpu_finish as gf
from hyperqueue_amd import abi
from hyperqueue_amd.core import TaskBuilder as TB
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _ctx(form, **kw):
    """a context of the form: "view" reads HQTICK_ORDERED_VIEW=1 when it is created (as tests/test_gpu_assigned_forms.py creates it)"""
    from hyperqueue_amd.tick import Tick

    env = {"HQTICK_ORDERED_VIEW": "1"} if form == "view" else {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Tick(abi.make_config(flags=abi.HQTICK_FLAG_CONSUME_IN_TICK if form == "in_tick" else 0, **{**lc.CFG, **kw}))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _play(form, seed):
    oracle = Oracle(abi.make_config(reserve=1, fill_max=2, **lc.CFG), canonical=True)
    a = _ctx(form, reserve=1, fill_max=2)
    try:
        given = lambda: Oracle(abi.make_config(reserve=1, fill_max=2, **lc.CFG))
        return lc.play(lc.history(seed, form), oracle, rc.DeviceSide(a, form, given))
    finally:
        a.close()


@pytest.mark.parametrize("form,seed", [(form, seed) for form in lc.FORMS for seed in lc.SEEDS[form]])
def test_history(form, seed):
    h = _play(form, seed)
    print(f"{form} seed {seed}: {len(h.log)} steps, {h.rounds_done} rounds" + (f", the tick of round {h.ended_early} refused" if h.ended_early is not None else ""))


@pytest.mark.parametrize("form", lc.FORMS)
def test_the_first_tick_after_a_lost_worker(form):
    """history view / 0 cut down to two steps: worker 53 of four is lost before the first tick.  The reference's worker map keeps its 8 buckets and the other
    workers their places in them; the resident worker set re-derived the iteration order from the three remaining ids (a map of 4 buckets), and
    process_proactive_filling walked the workers in another order: four PREFILL records went to the other one of workers 50 and 52"""
    oracle = Oracle(abi.make_config(reserve=1, fill_max=2, **lc.CFG), canonical=True)
    a = _ctx(form, reserve=1, fill_max=2)
    try:
        h = lc.history(0, "view", fixed=[("lose", 53), ("tick", None)])  # (that history's environment, ticked in each form)
        h.form = form
        lc.play(h, oracle, rc.DeviceSide(a, form))
        assert h.cov["PREFILL record"] >= 4 and len(h.env.workers) == 3
    finally:
        a.close()


@pytest.mark.parametrize("form", lc.FORMS)
def test_audit_mode_runs_a_history(form):
    """a context created with HQTICK_CHECK_RESIDENT=1 audits itself after every call that changes resident state: the form's first history runs through (a child
    process: the variable is read when the library creates the context)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_lifecycle as g\n"
            "h = g._play(%r, %d)\nprint('AUDITED-OK', len(h.log))\n") % (os.path.dirname(HERE), HERE, form, lc.SEEDS[form][0])
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HQTICK_CHECK_RESIDENT="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "AUDITED-OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- the zero-selection two-call tick
@pytest.mark.parametrize("how", ["consumed", "abandoned", "in_tick", "view"])
def test_a_tick_that_selects_nothing_still_enters_its_redirect(how):
    """prefilled tasks, an empty ready set and a new worker with room: the tick's whole output is a retract and a FROM_PREFILL redirect.  ReadySet::selected(0) left
    no live selection, Ledger::pending_live(false) then cleared the placement, and the consume entered nothing -- while the Retracting table had moved at tick
    time: the ledger kept the task prefilled on w1 and w2's row free.  Now the placement waits for the consume like any other, and a delta still drops it."""
    oracle = Oracle(abi.make_config(reserve=1, fill_max=1, **lc.CFG), canonical=True)
    form = {"consumed": "two_call", "abandoned": "two_call"}.get(how, how)
    a = _ctx(form, reserve=1, fill_max=1)
    try:
        def first(e, snap):
            a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
            return gf._tick(a, snap)

        def joined(e, wid):
            row = cc.free_rows(e)[sorted(e.workers).index(wid)][None, :]
            a.cluster_add_workers([wid], row, row)

        e, w1, w2, assigned, prefilled = lc.zero_selection_env(first, on_add_worker=joined)
        cc.seed_ready_graph(a, e)
        rc.state_matches(a, e)
        assert a.ready_count() == 0 and a.assigned_prefilled_count() == 1 and a.assigned_lookup([prefilled])[0].tolist() == [w1]
        snap = e.snapshot()
        want = oracle.tick(snap)
        lc.check_zero_selection_result(e, want, w1, w2, prefilled)
        free_before = a.assigned_free_rows().copy()
        rc.tick_equals(rc.tick_raw(a, snap), want)
        if form != "in_tick":
            ids = sorted(e.tasks)
            before = rc.digest(a, ids)
            row = cc.free_rows(e)[:1]
            for call in (lambda: a.start_tasks([assigned], [w1], [0], [e.tasks[assigned].rq], [e.tasks[assigned].priority]), lambda: a.finish_tasks([assigned], [w1]),
                         lambda: a.fail_tasks([assigned], [w1]), lambda: a.cancel_tasks([prefilled]), lambda: a.cluster_remove_workers([w2]),
                         lambda: a.cluster_add_workers([w2 + 1], row, row), lambda: a.assigned_release([assigned]),
                         lambda: a.retract_response(w1, [prefilled]), lambda: a.retracting_add([prefilled], [w1])):
                rc.expect_pending(call)
            assert rc.digest(a, ids) == before and (a.assigned_free_rows() == free_before).all()
            rc.state_matches(a, e, audit=rc.BETWEEN)  # nothing is state yet, the Retracting table included
            if how == "abandoned":  # a ready-set delta instead of the consume: the placement is dropped
                x = e.new_task(TB().cpus(2))  # (fits no worker)
                assert a.graph_add_tasks([x], [e.tasks[x].priority], [e.tasks[x].rq], [[]]).tolist() == [x]
                a.ready_consume_last()
                rc.state_matches(a, e)
                assert a.assigned_lookup([prefilled])[0].tolist() == [w1] and a.assigned_prefilled_count() == 1 and a.retracting_count() == 0
                assert (a.assigned_free_rows() == free_before).all()
                a.finish_tasks([assigned], [w1])  # (event calls go through again)
                e.finish_tasks([(assigned, w1)])
                rc.state_matches(a, e)
                snap = e.snapshot()
                want = oracle.tick(snap)
                rc.tick_equals(rc.tick_raw(a, snap), want)
            a.ready_consume_last()
        e.apply(want)
        if how != "abandoned":
            assert a.assigned_lookup([prefilled])[0].tolist() == [w2] and a.assigned_lookup([prefilled])[1].tolist() == [want.redirects[0][2]]
            assert a.assigned_prefilled_count() == 0 and a.retracting_count() == 1 and a.assigned_running([prefilled]).tolist() == [0]
        assert (a.assigned_free_rows() == want.new_free).all()
        rc.state_matches(a, e)  # (the audit with CROSS and STRICT among it)
        gf._ready_is(a, e)
    finally:
        a.close()
