"""One place for comparing a context's resident state with the SchedEnv mirror, and the device side of the lifecycle histories (tests/lifecycle_cases.py).
state_matches() is the whole comparison after a step: counts, free rows, every ledger entry with its running byte, multi-node workers, graph counters, worker
flags and the audit.  The helpers the single-call GPU tests grew (entries_match, ledger_matches, sanity_check_free) live here and are used from there under
their old names.  Not a test module."""
from __future__ import annotations

import numpy as np
import pytest

import cancel_cases as cc
from hyperqueue_amd import abi, core

AUDIT = abi.HQ_CHECK_ALL | abi.HQ_CHECK_STRICT
BETWEEN = abi.HQ_CHECK_READY | abi.HQ_CHECK_LEDGER | abi.HQ_CHECK_GRAPH  # what with_audit (csrc/hqtick.cpp) runs: the parts that hold after every single call
NO_ENTRY = 0xFF
GONE = 0xFFFFFFFF


def ready_total(e):
    return sum(len(s) for s in e.ready.values())


def running_want(e, ids):
    """the running byte per id as the mirror's states give it: Running 1; Assigned, Prefilled, multi-node and a Retracting task's entry on its redirect target
    (or on its own worker, retaken) 0; no entry 0xFF"""
    out = []
    for x in ids:
        t = e.tasks.get(x)
        if t is None or t.state in (core.WAITING, core.FINISHED):
            out.append(NO_ENTRY)
        elif t.state == core.RETRACTING:
            out.append(0 if x in e.redirects or x in e.retaken_variant else NO_ENTRY)
        else:
            out.append(1 if t.state == core.RUNNING else 0)
    return out


def entries_match(a, e):
    """running bytes, workers and variants of every id the mirror ever had"""
    ids = sorted(e.tasks)
    assert a.assigned_running(ids).tolist() == running_want(e, ids)
    lw, lv = a.assigned_lookup(ids)
    for x, w, v in zip(ids, lw.tolist(), lv.tolist()):
        t = e.tasks[x]
        if t.state in (core.ASSIGNED, core.RUNNING):
            assert (w, v) == (t.worker, t.rv), x
        elif t.state == core.PREFILLED:
            assert (w, v) == (t.worker, 0xFE), x
        elif t.state == core.RUNNING_MN:
            assert (w, v) == (t.mn_workers[0], 0xFF), x
    return ids, lw, lv


def ledger_matches(a, e):
    assert a.assigned_mn_count() == sum(1 for t in e.tasks.values() if t.state == core.RUNNING_MN)
    assert a.assigned_prefilled_count() == sum(1 for t in e.tasks.values() if t.state == core.PREFILLED)
    assert a.assigned_count() == sum(len(w.assigned_tasks) for w in e.workers.values())
    sn = [abi.HQ_WORKER_SN if e.workers[w].sn() else 0 for w in sorted(e.workers)]
    assert [f & abi.HQ_WORKER_SN for f in a.cluster_worker_flags().tolist()] == sn


def sanity_check_free(e):
    """Worker::sanity_check (server/worker.rs:236-271) on the SchedEnv mirror: resources.clone(), then remove(rq) per assigned task, against free_resources.
    -> the (worker id << 32 | resource) keys where they differ: the rows a saturating free.remove or an ALL-before-AMOUNT release has left over-full, which the
    reference's own check asserts on and the audit must report as HQ_INV_LEDGER_FREE -- exactly those, no others"""
    R, bad = e.n_resources, []
    for wid, w in e.workers.items():
        if not w.sn():
            continue
        want = list(w.total) + [0] * (R - len(w.total))
        for tid in w.assigned_tasks:
            for (r, kind, a) in e._variant(e.tasks[tid].rq, e._assigned_variant(tid, wid))["entries"]:
                want[r] = max(0, want[r] - a) if kind == abi.HQ_ENTRY_AMOUNT else 0
        have = list(w.free) + [0] * (R - len(w.free))
        bad += [wid << 32 | r for r in range(R) if want[r] != have[r]]
    return bad


def audit_matches(a, e, parts=AUDIT):
    """the audit fails nothing -- but HQ_INV_LEDGER_FREE at exactly the rows where the mirror's own free amounts are not what its tasks leave (above the worker's
    total after an ALL-before-AMOUNT release: `overfull` in the single-call tests).  The lifecycle histories draw no over-committing start (tests/lifecycle_cases.py
    says why), so with them `bad` is always empty and this is the plain "fails nothing": the over-full branch is exercised by tests/test_gpu_audit.py alone"""
    bad = sanity_check_free(e)
    rep = a.resident_check(parts)
    assert rep["failed"] == ({"HQ_INV_LEDGER_FREE": (len(bad), min(bad))} if bad else {}), rep["failed"]
    return rep


def state_matches(a, e, audit=AUDIT):
    """everything resident against the mirror; every figure is an integer, so every comparison is exact"""
    assert a.ready_count() == ready_total(e)
    assert (a.assigned_free_rows() == cc.free_rows(e)).all()
    ledger_matches(a, e)
    assert a.retracting_count() == sum(1 for t in e.tasks.values() if t.state == core.RETRACTING)
    ids, lw, lv = entries_match(a, e)
    for x, w, v in zip(ids, lw.tolist(), lv.tolist()):
        t = e.tasks[x]
        if t.state == core.RETRACTING:  # its entry is the redirect's, on the target; put back on its own worker: there; still in its queue: none
            want = e.redirects[x] if x in e.redirects else (t.worker, e.retaken_variant[x]) if x in e.retaken_variant else (abi.HQ_NO_WORKER, NO_ENTRY)
            assert (w, v) == tuple(want), x
        elif t.state in (core.WAITING, core.FINISHED):
            assert (w, v) == (abi.HQ_NO_WORKER, NO_ENTRY), x
        elif t.state == core.RUNNING_MN:
            assert a.assigned_mn_workers(x) == [t.mn_workers[0]] + sorted(t.mn_workers[1:]), x
    assert a.graph_unfinished(ids).tolist() == [GONE if e.tasks[x].state == core.FINISHED else e.tasks[x].unfinished_deps for x in ids]
    assert a.cluster_workers().tolist() == sorted(e.workers)
    if audit:
        audit_matches(a, e, audit)


def digest(a, ids):
    """what a refused call must leave as it was"""
    s = a.graph_stats(); s.pop("last_kernel_us", None)
    lw, lv = a.assigned_lookup(ids)
    return dict(ready=a.ready_count(), graph=s, sn=a.assigned_count(), pf=a.assigned_prefilled_count(), mn=a.assigned_mn_count(), retr=a.retracting_count(),
                free=a.assigned_free_rows().tolist(), worker=lw.tolist(), variant=lv.tolist(), run=a.assigned_running(ids).tolist(), unf=a.graph_unfinished(ids).tolist(),
                workers=a.cluster_workers().tolist(), flags=a.cluster_worker_flags().tolist())


def tick_raw(a, snap):
    """a tick of a ledger context on its resident ready set: resident workers and Retracting table, no assigned and no prefilled CSR"""
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None; sc.prefilled_off = None; sc.prefilled_rq = None
    sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None
    sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
    return abi.parse_result(a.tick_raw(sc, resident=True), len(snap.worker_id), snap.n_resources)


def tick_equals(got, want):
    assert got.status == want.status
    assert got.counts == want.counts, dict(canonical=(got.is_canonical, want.is_canonical), optimal=(got.is_optimal, want.is_optimal), got=got.counts, want=want.counts)
    flags = dict(canonical=(got.is_canonical, want.is_canonical), optimal=(got.is_optimal, want.is_optimal))
    assert got.records == want.records, dict(flags, differ=[(w, sorted(set(a) ^ set(b))) for w, (a, b) in enumerate(zip(got.records, want.records)) if a != b])
    assert got.retracts == want.retracts, dict(flags, got=got.retracts, want=want.retracts)
    # (the redirects as a set with their kinds: the order of the list follows the reference's Map iteration and is no part of the result -- tests/test_gpu_parity.py,
    # tests/test_host_stages.py and tests/test_gpu_fuzz.py compare them the same way)
    assert sorted(zip(got.redirects, got.redirect_kinds)) == sorted(zip(want.redirects, want.redirect_kinds)), dict(flags, got=(got.redirects, got.redirect_kinds), want=(want.redirects, want.redirect_kinds))
    assert got.mn == want.mn
    assert (np.asarray(got.new_free) == np.asarray(want.new_free)).all()


def expect_pending(call):
    from hyperqueue_amd.tick import HqTickError

    with pytest.raises(HqTickError) as err:
        call()
    assert err.value.code == abi.HQTICK_E_INVALID and "pending" in str(err.value), str(err.value)


class DeviceSide:
    """the lifecycle driver's calls on context a: each step's own answer against the mirror's (which the driver has applied already), then state_matches()"""

    def __init__(self, a, form, given=None):
        self.a, self.two_call, self.given = a, form != "in_tick", given  # given: () -> an oracle for tick_given

    def seed(self, e):
        a = self.a
        a.cluster_upload(e.snapshot()); a.assigned_enable([]); a.assigned_track_prefilled([])
        cc.seed_ready_graph(a, e)
        state_matches(a, e)

    def tick(self, e, snap, want, code):
        from hyperqueue_amd.tick import HqTickError

        try:
            got = tick_raw(self.a, snap)
        except HqTickError as err:
            assert code < 0 and err.code == code, (err.code, code, str(err))
            return
        assert code >= 0, f"the reference refuses this tick with {code}, the library returned status {got.status}"
        if not got.is_canonical and self.given:
            # optimal, but the tie-break ran out of its budget (hqtick_result.is_canonical = 0): the claim is the reference's own mapping of THIS placement
            # (Oracle.tick_given, as tests/test_host_stages.py and smoke() take it), and the mirror goes on from it
            assert got.is_optimal and want.is_optimal
            want = self.given().tick_given(snap, got.counts, is_optimal=True)
        tick_equals(got, want)
        if self.two_call:  # nothing has become state yet: the mirror is the one before the tick
            state_matches(self.a, e, audit=BETWEEN)
        return want

    def refused(self, e, which):
        a, ids = self.a, sorted(e.tasks)
        held = [x for x in ids if e.tasks[x].state in (core.ASSIGNED, core.RUNNING, core.PREFILLED)][:3] or ids[:1]
        ws = [e.tasks[x].worker if e.tasks[x].worker is not None else sorted(e.workers)[0] for x in held]
        before = digest(a, ids)
        if which == "start":
            call = lambda: a.start_tasks(held, ws, [0] * len(held), [e.tasks[x].rq for x in held], [e.tasks[x].priority for x in held])
        elif which == "finish":
            call = lambda: a.finish_tasks(held, ws)
        elif which == "fail":
            call = lambda: a.fail_tasks(held, ws)
        elif which == "cancel":
            call = lambda: a.cancel_tasks(held)
        elif which == "lose":
            call = lambda: a.cluster_remove_workers([sorted(e.workers)[0]])
        elif which == "retract":  # (the Retracting table's part of the tick waits with the placement: a response now would meet the table of before the tick)
            call = lambda: a.retract_response(sorted(e.workers)[0], held)
        else:
            row = cc.free_rows(e)[:1]
            call = lambda: a.cluster_add_workers([max(e.workers) + 1000], row, row)
        expect_pending(call)
        assert digest(a, ids) == before

    def consume(self, e, want):
        self.a.ready_consume_last()

    def new_tasks(self, e, ids, deps):
        ts = [e.tasks[x] for x in ids]
        now = self.a.graph_add_tasks(ids, [t.priority for t in ts], [t.rq for t in ts], [deps[x] for x in ids])
        assert now.tolist() == [x for x in ids if e.tasks[x].unfinished_deps == 0]

    def disposed(self, e, msgs):
        """process_retracted (server/reactor.rs:34-62), the host's part: the tasks leave the prefilled entries, are Retracting{worker} and back in their queue"""
        a = self.a
        msgs = sorted((x, w) for (w, x) in msgs)
        ids = [x for x, _ in msgs]
        assert a.assigned_unprefill(ids) == len(ids)
        a.retracting_add(ids, [w for _, w in msgs])
        a.ready_add(ids, [e.tasks[x].priority for x in ids], [e.tasks[x].rq for x in ids])

    def start(self, e, triples, accepted):
        ids = [t[0] for t in triples]
        got = self.a.start_tasks(ids, [t[1] for t in triples], [t[2] for t in triples], [e.tasks[x].rq if x in e.tasks else 0 for x in ids],
                                 [e.tasks[x].priority if x in e.tasks else 0 for x in ids])
        assert got["kind"].tolist() == e.last_start_kinds
        assert got["accepted"] == accepted == sum(k in abi.HQ_START_ACCEPTED for k in e.last_start_kinds) and self.a.assigned_last_unknown() == len(triples) - accepted

    def finish(self, e, pairs, released):
        got = self.a.finish_tasks([p[0] for p in pairs], [p[1] for p in pairs])
        kinds = e.last_finish_kinds
        assert got["kind"].tolist() == kinds
        n_acc = sum(k in abi.HQ_FINISH_ACCEPTED for k in kinds)
        assert got["accepted"] == n_acc and self.a.assigned_last_unknown() == len(pairs) - n_acc
        assert got["released"].tolist() == sorted(released) and got["graph_unknown"] == 0

    def fail(self, e, pairs, accepted):
        got = self.a.fail_tasks([p[0] for p in pairs], [p[1] for p in pairs])
        kinds, lists = e.last_fail_kinds, e.last_fail_consumers
        assert got["kind"].tolist() == kinds
        assert got["accepted"] == accepted == sum(k in abi.HQ_FAIL_ACCEPTED for k in kinds) and self.a.assigned_last_unknown() == len(pairs) - accepted
        off = got["consumer_off"].tolist()
        assert len(off) == len(pairs) + 1 and off[0] == 0
        assert [got["consumer_id"][off[k]:off[k + 1]].tolist() for k in range(len(pairs))] == lists  # fail's consumer CSR (fail_last)
        roots = [p[0] for p, k in zip(pairs, kinds) if k in abi.HQ_FAIL_ACCEPTED]
        assert got["removed"].tolist() == sorted(roots + [c for l in lists for c in l]) and got["graph_unknown"] == 0

    def cancel(self, e, ids, messages, closure):
        got = self.a.cancel_tasks(ids)
        routes = e.last_cancel_routes
        assert got["messages"] == {w: xs for w, xs in sorted(messages.items())}
        assert got["n_ids"] == sum(len(v) for v in messages.values())
        assert got["route_worker"].tolist() == [abi.HQ_NO_WORKER if w is None else w for (w, _) in routes]
        assert got["route_kind"].tolist() == [k for (_, k) in routes]
        assert got["closure"].tolist() == closure

    def retract(self, e, wid, ids, want, n_left):
        assert sorted(self.a.retract_response(wid, ids)) == sorted(want)
        assert self.a.last_retract_left == n_left

    def lose(self, e, wid, info):
        a = self.a
        assert a.cluster_remove_workers([wid]) == info["sent"]
        assert a.cluster_last_requeued_running() == e.last_lost_running
        requeued = a.cluster_last_requeued()
        back = {x for s in e.ready.values() for x in s} - info["ready_before"] - set(info["disposed"])
        assert [x[0] for x in requeued] == sorted(back) and set(e.last_lost_running) <= back
        assert [(x[1], x[2]) for x in requeued] == [(e.tasks[x[0]].rq, e.tasks[x[0]].priority) for x in requeued]
        assert a.cluster_last_requeued_prefilled() == info["prefilled"]

    def add_worker(self, e, wid):
        row = cc.free_rows(e)[sorted(e.workers).index(wid)][None, :]
        self.a.cluster_add_workers([wid], row, row)

    def check(self, e):
        state_matches(self.a, e)

    def end(self, e):
        """the resident ready set holds exactly the mirror's ids (destructive: last)"""
        a = self.a
        ready = sorted(x for s in e.ready.values() for x in s)
        assert a.ready_count() == len(ready)
        if ready:
            assert a.ready_remove(ready) == len(ready)
        assert a.ready_count() == 0
