"""hqtick_reject_tasks, hqtick_cluster_enable_request and hqtick_cluster_blocked (include/hqtick.h) on the device: the reference's task_reject
scenarios through graph + ready set + ledger with prefilled tracking + the resident Retracting table and blocked sets, with the resident ticks that follow them;
every kind in one batch; the claim decided by position at wave and workgroup edges; twin contexts (the one call against hqtick_assigned_release +
hqtick_assigned_unprefill + hqtick_ready_add + hqtick_cluster_set_blocked driven by the mirror) at batch sizes around those edges; the requeue's order and the
merge's three starting states; the batch order under saturating arithmetic; the claim words; the call's rules; the blocked-set accessors without a ledger; the
audit mode; the seeded histories of tests/reject_cases.py in the three forms of the lifecycle test; one larger batch."""
import copy
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import cancel_cases as cc
import reject_cases as rj
import resident_checks as rc
import test_gpu_finish as gf
import test_gpu_lifecycle as gl
import test_gpu_start as gs
from hyperqueue_amd import abi, core, workloads
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

CFG = dict(time_limit_s=20.0)
ACC = abi.HQ_REJECT_ACCEPTED
K = abi
NO_ENTRY = 0xFF
_ctx, _tick, _clean, _prefill_by_hand = gs._ctx, gf._tick, gf._clean, gs._prefill_by_hand


def _blocked_match(a, e):
    for w in sorted(e.workers):
        assert sorted(a.cluster_blocked(w)) == sorted(e.workers[w].blocked_requests), w


def _cols(e, triples):
    """the four columns of the call: ids, reporters, variants (None: no variant) and the tasks' own requests (0 for an id the mirror does not know)"""
    ids = [t[0] for t in triples]
    return ids, [t[1] for t in triples], [t[2] for t in triples], [e.tasks[x].rq if x in e.tasks else 0 for x in ids]


def _answer_matches(got, e, triples, want):
    kinds = e.last_reject_kinds
    assert got["kind"].tolist() == kinds
    assert got["accepted"] == want == sum(k in ACC for k in kinds)
    assert got["requeued"] == e.last_reject_requeued
    assert got["reassigned"] == e.last_reject_reassigned


def _disposed(a, e, mark):
    """process_retracted for the prefill sets the requeued tasks dissolved (the host's part, as resident_checks.DeviceSide.disposed)"""
    msgs = e.retract_messages[mark:]
    if msgs:
        rc.DeviceSide(a, "two_call").disposed(e, msgs)


def _reject_checked(a, e, triples, audit=rc.AUDIT):
    """the batch on the mirror and on context a: kinds, accepted and refused counts, the requeued and reassigned lists, then the whole resident state and the blocked
    sets.  Free rows above a worker's total (an ALL entry released before AMOUNT entries) are the mirror's too: resident_checks.audit_matches expects exactly those"""
    mark = len(e.retract_messages)
    want = e.reject_tasks(triples)
    got = a.reject_tasks(*_cols(e, triples))
    print("kinds", got["kind"].tolist(), "accepted", got["accepted"], "requeued", len(got["requeued"]))
    _answer_matches(got, e, triples, want)
    assert a.assigned_last_unknown() == len(triples) - want
    _disposed(a, e, mark)
    rc.state_matches(a, e, audit)
    _blocked_match(a, e)
    return got


class DevSide:
    """reject_cases' `side` on a context: every tick is a two-call tick on the resident ready set, compared with the CPU oracle's on the mirror's snapshot"""

    def __init__(self, a, e, **cfg):
        self.a, self.e, self.oracle = a, e, Oracle(abi.make_config(**{**CFG, **cfg}), canonical=True)

    def schedule(self):
        a, e = self.a, self.e
        snap = e.snapshot()
        res = _tick(a, snap, resident=True)
        rc.tick_equals(res, self.oracle.tick(snap))
        a.ready_consume_last(); e.apply(res)
        rc.state_matches(a, e)

    def reject(self, triples):
        return _reject_checked(self.a, self.e, triples)["kind"].tolist()

    def enable(self, wid, rq, v):
        was = self.a.cluster_enable_request(wid, rq, v)
        self.e.enable_request(wid, rq, v)
        _blocked_match(self.a, self.e)
        return was


def _first_tick(a, e):
    """the worker set, the ledger and one tick on the snapshot's own ready set, then graph and resident ready set from the mirror"""
    snap = e.snapshot()
    a.cluster_upload(snap); a.assigned_enable([]); a.assigned_track_prefilled([])
    e.apply(_tick(a, snap))
    cc.seed_ready_graph(a, e)
    rc.state_matches(a, e)


# ---------------------------------------------------------------------------------------------- 1: the reference's scenarios
def _run_reject1(a):
    e = SchedEnv(abi.make_config(**CFG))
    w, t = rj.setup_reject1(e)
    _first_tick(a, e)
    rj.act_reject1(DevSide(a, e), e, w, t)
    return e


def test_task_reject1():
    a = _ctx()
    try:
        _run_reject1(a)
    finally:
        a.close()


def test_task_reject2():
    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        w, t = rj.setup_reject2(e)
        _first_tick(a, e)
        rj.act_reject2(DevSide(a, e), e, w, t)
        assert a.assigned_lookup([t])[1].tolist() == [1] and a.cluster_blocked(w) == [(e.tasks[t].rq, 0)]
    finally:
        a.close()


def test_task_reject3():
    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        w, t1, t2 = rj.setup_reject3(e)
        _first_tick(a, e)
        rj.act_reject3(DevSide(a, e), e, w, t1, t2)
        assert a.assigned_count() == 0 and a.ready_count() == 2 and a.cluster_blocked(w) == [(e.tasks[t1].rq, 0)]
    finally:
        a.close()


def test_prefill_rejected():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e = SchedEnv(abi.make_config(reserve=1, fill_max=1, **CFG))
        tasks = e.new_tasks(3, TB())
        w1 = e.new_worker(WB(1))
        _first_tick(a, e)
        prefilled = next(x for x in tasks if e.task(x).is_prefilled())
        rj.act_prefill_rejected(DevSide(a, e, reserve=1, fill_max=1), e, w1, prefilled)
        assert a.assigned_prefilled_count() == 0 and a.assigned_count() == 1 and a.ready_count() == 2
    finally:
        a.close()


def test_steal_rejected():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e, w1, w2, t, others = gf._retracting_pair(a)
        cc.seed_ready_graph(a, e)
        free = a.assigned_free_rows().copy()
        rj.act_steal_rejected(DevSide(a, e, reserve=1, fill_max=1), e, w1, w2, t)
        assert a.retracting_count() == 0 and a.assigned_lookup([t])[0].tolist() == [w2] and (a.assigned_free_rows() == free).all()
        gf._next_tick_equals_the_mirrors(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 2: every kind in one batch
def test_every_kind_in_one_batch():
    a = _ctx(reserve=1, fill_max=1)
    try:
        e, ws, t = gf._kinds_env(a, None)
        w1, w2, w3, root, node = ws
        sn = t["sn"]
        gs._start_checked(a, e, [(sn[2], w3, 0)])
        triples = [(sn[0], root, 0), (sn[0], w3, None), (sn[0], w3, 3), (sn[0], w3, 0), (sn[0], w3, 0), (sn[2], w3, 0), (t["red"], w2, 0), (t["red"], w1, 9), (t["red"], w1, 0),
                   (t["red"], w1, 0), (10**12, w1, 0), (t["pf"], w3, None), (t["pf"], w3, 0), (t["q"], w3, 0), (t["q"], w3, 0), (t["waiting"], w3, 0), (t["mn"], root, 0),
                   (sn[1], rj.GHOST, 0)]
        want = [K.HQ_REJECT_WRONG_WORKER, K.HQ_REJECT_WRONG_VARIANT, K.HQ_REJECT_BAD_VARIANT, K.HQ_REJECT_ASSIGNED, K.HQ_REJECT_REPEAT, K.HQ_REJECT_RUNNING, K.HQ_REJECT_WRONG_WORKER,
                K.HQ_REJECT_BAD_VARIANT, K.HQ_REJECT_REDIRECTED, K.HQ_REJECT_REPEAT, K.HQ_REJECT_NONE, K.HQ_REJECT_PREFILLED, K.HQ_REJECT_REPEAT, K.HQ_REJECT_RETRACTING,
                K.HQ_REJECT_REPEAT, K.HQ_REJECT_NONE, K.HQ_REJECT_MN, K.HQ_REJECT_WRONG_WORKER]
        n_ready = a.ready_count()
        got = _reject_checked(a, e, triples)
        assert got["kind"].tolist() == want and set(want) == set(range(11)) and got["accepted"] == 4
        assert a.ready_count() == n_ready + 2  # sn[0] and the prefilled task; the Retracting task in its queue is not added a second time
        assert [x[0] for x in got["requeued"]] == sorted([sn[0], t["pf"]]) and got["reassigned"] == [(t["red"], w2, 0)]
        assert a.retracting_count() == 0 and a.assigned_prefilled_count() == 0 and a.assigned_lookup([t["red"], sn[0], t["pf"]])[0].tolist() == [w2, abi.HQ_NO_WORKER, abi.HQ_NO_WORKER]
        rq, rq_red = e.tasks[sn[0]].rq, e.tasks[t["red"]].rq
        assert e.tasks[t["q"]].rq == rq  # (the Retracting task in its queue blocks the pair w3 has blocked already)
        assert {w: a.cluster_blocked(w) for w in (root, w1, w2, w3, node)} == {root: [(rq, 0)], w1: [(rq_red, 0)], w2: [(rq_red, 0)], w3: [(rq, 0)], node: []}
        gf._ready_is(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 3: the claim goes to the lower position
def test_claim_by_position_not_by_arrival():
    """two eligible positions of one prefilled id that reject different variants, at both sides of a wavefront and a workgroup edge and in two workgroups, in both
    orders: the lower position is _PREFILLED and its pair is the one blocked, the other position is a repeat and blocks nothing"""
    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        (w,) = e.new_workers_cpus([64])
        two = TB().cpus(2).next_variant().cpus(1)
        cases = [(p, q, first) for (p, q) in ((0, 1), (63, 64), (255, 256), (0, 256)) for first in (0, 1)]
        pf = [e.new_task(two) for _ in cases]
        for x in pf:
            _prefill_by_hand(e, x, w)
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        rq = e.tasks[pf[0]].rq
        for x, (p, q, first) in zip(pf, cases):
            triples = [(10**12 + k, w, 0) for k in range(257)]
            triples[p] = (x, w, first); triples[q] = (x, w, 1 - first)
            got = _reject_checked(a, e, triples)
            kinds = got["kind"].tolist()
            assert kinds[p] == K.HQ_REJECT_PREFILLED and kinds[q] == K.HQ_REJECT_REPEAT and got["accepted"] == 1
            assert a.cluster_blocked(w) == [(rq, first)] and got["requeued"] == [(x, rq, e.tasks[x].priority)]
            a.cluster_set_blocked(w, []); e.workers[w].blocked_requests.clear()
        assert a.assigned_prefilled_count() == 0 and a.ready_count() == len(pf)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 4: batch sizes at the edges, twin contexts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_against_the_parents_sequence(n):
    """a random batch of n positions with refused ones among them; context A takes the one call, context B the parent's sequence for the positions the mirror
    accepted -- hqtick_assigned_release, hqtick_assigned_unprefill, hqtick_retract_response, hqtick_ready_add -- and hqtick_cluster_set_blocked with every worker's
    whole list; ledger, free rows, ready set and blocked pairs agree"""
    rng = np.random.default_rng(9100 + n)
    a, b = _ctx(), _ctx()
    try:
        e, ws = gs._mixed_env(rng, n, (a, b))
        pool = sorted(e.tasks)
        triples = []
        for _ in range(n):
            x = pool[int(rng.integers(0, len(pool)))]
            t = e.tasks[x]
            u = rng.random()
            w = t.worker if t.worker is not None and u < 0.8 else ws[int(rng.integers(0, 3))]
            v = (t.rv if t.state == core.ASSIGNED else 0) if rng.random() < 0.8 else (None, 0, 1, 2)[int(rng.integers(0, 4))]
            triples.append((x, w, v) if u < 0.95 else (10**12 + int(rng.integers(0, 9)), w, 0))
        got = _reject_checked(a, e, triples)
        kinds = got["kind"].tolist()
        if n >= 63:
            assert any(k not in ACC for k in kinds) and K.HQ_REJECT_ASSIGNED in kinds and K.HQ_REJECT_PREFILLED in kinds
        rel = [x for (x, w, v), k in zip(triples, kinds) if k == K.HQ_REJECT_ASSIGNED]
        unp = [x for (x, w, v), k in zip(triples, kinds) if k == K.HQ_REJECT_PREFILLED]
        assert b.assigned_release(rel) == len(rel) and b.assigned_unprefill(unp) == len(unp)
        for (x, w, v), k in zip(triples, kinds):
            if k in (K.HQ_REJECT_RETRACTING, K.HQ_REJECT_REDIRECTED):
                b.retract_response(w, [x])
        back = sorted(rel + unp)
        b.ready_add(back, [e.tasks[x].priority for x in back], [e.tasks[x].rq for x in back])
        for w in ws:
            b.cluster_set_blocked(w, sorted(e.workers[w].blocked_requests))
        assert got["requeued"] == [(x, e.tasks[x].rq, e.tasks[x].priority) for x in back]
        ids = sorted(e.tasks)
        va, vb = (dict(ready=t.ready_count(), sn=t.assigned_count(), pf=t.assigned_prefilled_count(), retr=t.retracting_count(), free=t.assigned_free_rows().tolist(),
                       worker=t.assigned_lookup(ids)[0].tolist(), variant=t.assigned_lookup(ids)[1].tolist(), blocked=[sorted(t.cluster_blocked(w)) for w in ws]) for t in (a, b))
        assert va == vb
        _clean(b)
        ready = sorted(x for s in e.ready.values() for x in s)
        for t in (a, b):  # the ready sets hold the same ids: every one of them leaves both, and nothing is left
            assert t.ready_remove(ready) == len(ready) and t.ready_count() == 0
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 5: the requeue's order and the merge
def _held_env(a, n_assigned, n_pf, n_ready, interleave=False):
    """one large worker; tasks assigned, prefilled and ready.  interleave: the kinds alternate over the ids, so that the requeued ids lie below, between and above
    the resident ones"""
    e = SchedEnv(abi.make_config(**CFG))
    (w,) = e.new_workers_cpus([4000])
    kinds = ["a"] * n_assigned + ["p"] * n_pf + ["r"] * n_ready
    if interleave:
        kinds = [kinds[(j * 7) % len(kinds)] for j in range(len(kinds))] if np.gcd(7, len(kinds)) == 1 else kinds
        kinds[0], kinds[-1] = "a", "p"  # (an id below and an id above every resident one)
    out = dict(a=[], p=[], r=[])
    for k in kinds:
        x = e.new_task(TB().cpus(1))
        out[k].append(x)
        if k == "a":
            e.assign_task(x, w)
        elif k == "p":
            _prefill_by_hand(e, x, w)
    cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
    return e, w, out


@pytest.mark.parametrize("order", ["descending", "shuffled"])
@pytest.mark.parametrize("start", ["empty", "tombstones", "interleaved"])
def test_requeue_order_and_merge(order, start):
    """the requeued columns come out ascending whatever order the batch names the ids in, and the merge takes them into an empty resident set, into one that holds
    tombstones only, and between resident ids"""
    a = _ctx()
    try:
        e, w, ids = _held_env(a, 180, 121, 150 if start == "interleaved" else 0, interleave=start == "interleaved")
        n_ready = len(ids["r"])
        # (the graph released every task into the ready set and the held ones were removed again: without ready tasks the columns hold tombstones only)
        if start == "empty":
            a.ready_compact()  # ... and after a compaction nothing at all
        assert a.ready_count() == n_ready
        back = sorted(ids["a"] + ids["p"])
        if start == "interleaved":
            assert back[0] < min(ids["r"]) and back[-1] > max(ids["r"]) and any(min(ids["r"]) < x < max(ids["r"]) for x in back)
        batch = back[::-1] if order == "descending" else [back[int(k)] for k in np.random.default_rng(5).permutation(len(back))]
        triples = [(x, w, 0) for x in batch]
        got = _reject_checked(a, e, triples)
        assert got["accepted"] == len(back) and [x[0] for x in got["requeued"]] == back
        assert got["requeued"] == [(x, e.tasks[x].rq, e.tasks[x].priority) for x in back]
        assert a.ready_count() == len(back) + n_ready and a.assigned_count() == 0 and a.assigned_prefilled_count() == 0
        gf._ready_is(a, e)
    finally:
        a.close()


def test_a_retracting_position_leaves_the_ready_count_unchanged():
    a = _ctx()
    try:
        e, w, ids = _held_env(a, 3, 0, 4)
        t = ids["r"][1]
        e.tasks[t].state, e.tasks[t].worker = core.RETRACTING, w  # as process_retracted leaves it: in its queue
        a.retracting_add([t], [w])
        got = _reject_checked(a, e, [(t, w, 0), (ids["a"][0], w, 0), (t, w, 0)])
        assert got["kind"].tolist() == [K.HQ_REJECT_RETRACTING, K.HQ_REJECT_ASSIGNED, K.HQ_REJECT_REPEAT]
        assert a.ready_count() == 5 and a.retracting_count() == 0 and [x[0] for x in got["requeued"]] == [ids["a"][0]]
        gf._ready_is(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 6: the batch order under saturation
@pytest.mark.parametrize("order", ["all_first", "amounts_first"])
def test_order_under_saturation(order):
    """a cpus_all task and two 1-cpu tasks on one 4-cpu worker, all rejected in one batch.  ALL first: free = total = 4, then + 1 + 1 = 6 (above the total, as
    in the reference, workerload.rs:194-202); the AMOUNTs first: 1, 2, then ALL sets the total: 4.  The device follows the batch order as the reference's loop does."""
    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        (w,) = e.new_workers_cpus([4])
        one = [e.new_task(TB().cpus(1)) for _ in range(2)]
        big = e.new_task(TB().cpus_all())
        for x in one:
            e.assign_task(x, w)
        e.assign_task(big, w)
        assert e.workers[w].free[0] == 0
        cc.seed_ledger(a, e); cc.seed_ready_graph(a, e)
        batches = {"all_first": [(big, w, 0)] + [(x, w, 0) for x in one], "amounts_first": [(x, w, 0) for x in one] + [(big, w, 0)]}
        ends = {}
        for name, batch in batches.items():
            m = copy.deepcopy(e)
            assert m.reject_tasks(batch) == 3
            ends[name] = m.workers[w].free[0]
        assert ends == {"all_first": core.amount(6), "amounts_first": core.amount(4)}  # the two orders differ: the test means something
        got = _reject_checked(a, e, batches[order])
        assert got["kind"].tolist() == [K.HQ_REJECT_ASSIGNED] * 3
        assert int(a.assigned_free_rows()[0, 0]) == ends[order] == e.workers[w].free[0]
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 7: the claim words
def test_claim_words_are_restored():
    """the same batch twice: the entries of the first have left, so the second finds none -- and ids entered again behind it are claimed by a batch that names them
    at HIGHER positions than the one that took them out, which a claim word left behind would beat"""
    a = _ctx()
    try:
        e, w, ids = _held_env(a, 70, 70, 0)
        first = [(x, w, 0) for x in ids["a"] + ids["p"]]
        got = _reject_checked(a, e, first)
        assert got["accepted"] == 140
        got = _reject_checked(a, e, first)
        assert got["kind"].tolist() == [K.HQ_REJECT_NONE] * 140 and got["accepted"] == 0 and got["requeued"] == []
        a.cluster_set_blocked(w, []); e.workers[w].blocked_requests.clear()
        again = ids["a"][:40]
        for x in again:
            e.assign_task(x, w)
        assert a.ready_remove(again) == 40
        assert a.assigned_add([(x, w, e.tasks[x].rq, 0, e.tasks[x].priority) for x in again]) == 40
        pad = [(10**12 + j, w, 0) for j in range(300)]
        got = _reject_checked(a, e, pad + [(x, w, 0) for x in again])
        assert got["kind"].tolist() == [K.HQ_REJECT_NONE] * 300 + [K.HQ_REJECT_ASSIGNED] * 40
        gf._ready_is(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 8: the call's rules
def test_call_rules():
    from hyperqueue_amd.tick import HqTickError

    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        ws = e.new_workers_cpus([4, 4])
        held = [e.new_task(TB().cpus(1)) for _ in range(2)]
        e.assign_task(held[0], ws[0]); e.assign_task(held[1], ws[1])
        queued = [e.new_task(TB().cpus(1)) for _ in range(5)]
        with pytest.raises(HqTickError) as err:  # no resident ready set
            a.reject_tasks(held, ws, [0, 0])
        assert err.value.code == abi.HQTICK_E_INVALID
        a.cluster_upload(e.snapshot())
        cc.seed_ready_graph(a, e)
        n_ready = a.ready_count()
        with pytest.raises(HqTickError) as err:  # ledger off
            a.reject_tasks(held, ws, [0, 0])
        assert err.value.code == abi.HQTICK_E_INVALID and "assignment ledger not enabled" in str(err.value)
        assert a.ready_count() == n_ready and a.cluster_blocked(ws[0]) == []
        cc.seed_ledger(a, e)
        ids = sorted(e.tasks)
        before = rc.digest(a, ids)
        f = a._lib.hqtick_reject_tasks
        f.argtypes = [C.c_void_p, C.c_uint32, abi.u64p, abi.u32p, abi.u8p, abi.u32p]
        tid = np.asarray(held, np.uint64); wid = np.asarray(ws, np.uint32); var = np.zeros(2, np.uint8); rq = np.zeros(2, np.uint32)
        p = lambda x, ty: x.ctypes.data_as(ty)
        for args in ((None, p(wid, abi.u32p), p(var, abi.u8p)), (p(tid, abi.u64p), None, p(var, abi.u8p)), (p(tid, abi.u64p), p(wid, abi.u32p), None)):  # a null array
            assert f(a._ctx, 2, *args, p(rq, abi.u32p)) == abi.HQTICK_E_INVALID
        assert f(a._ctx, (1 << 26) + 1, p(tid, abi.u64p), p(wid, abi.u32p), p(var, abi.u8p), None) == abi.HQTICK_E_CAPACITY  # (refused before anything is read)
        assert rc.digest(a, ids) == before and all(a.cluster_blocked(w) == [] for w in ws)
        # rq may be NULL while the Retracting table is empty, and not once it holds a task
        a.retracting_add([queued[0]], [ws[0]]); e.tasks[queued[0]].state, e.tasks[queued[0]].worker = core.RETRACTING, ws[0]
        before = rc.digest(a, ids)
        assert f(a._ctx, 2, p(tid, abi.u64p), p(wid, abi.u32p), p(var, abi.u8p), None) == abi.HQTICK_E_INVALID
        assert rc.digest(a, ids) == before and all(a.cluster_blocked(w) == [] for w in ws)
        got = a.reject_tasks([], [], [])  # n = 0: an empty kind list
        assert got["accepted"] == 0 and len(got["kind"]) == 0 and got["requeued"] == [] and a.assigned_last_unknown() == 0
        assert rc.digest(a, ids) == before
        got = _reject_checked(a, e, [(queued[0], ws[0], 0)])  # ... with its request the Retracting task in its queue is Waiting again
        assert got["kind"].tolist() == [K.HQ_REJECT_RETRACTING] and a.retracting_count() == 0
        got = a.reject_tasks([held[1]], [ws[1]], [0])  # the table is empty again: NULL rq
        assert got["kind"].tolist() == [K.HQ_REJECT_ASSIGNED]
        e.reject_tasks([(held[1], ws[1], 0)])
        rc.state_matches(a, e); _blocked_match(a, e)
        for w in ws:  # (both workers have blocked the one request by now: enabled, so that the tick below places something)
            for (q, v) in sorted(e.workers[w].blocked_requests):
                assert a.cluster_enable_request(w, q, v) == 1
                e.enable_request(w, q, v)
        # a two-call tick's placement is pending: refused, nothing changes, and the consume still finds its selection
        res = _tick(a, e.snapshot(), resident=True)
        assert sum(len(r) for r in res.records) > 0
        before = rc.digest(a, ids)
        rc.expect_pending(lambda: a.reject_tasks(held, ws, [0, 0]))
        assert rc.digest(a, ids) == before
        a.ready_consume_last(); e.apply(res)
        rc.state_matches(a, e)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 9: the blocked set without a ledger
def test_blocked_set_accessors_without_the_ledger():
    from hyperqueue_amd.tick import HqTickError

    a = _ctx()
    try:
        e = SchedEnv(abi.make_config(**CFG))
        ws = e.new_workers_cpus([4, 4])
        e.rq_id(TB().cpus(1)); e.rq_id(TB().cpus(2).next_variant().cpus(1))
        with pytest.raises(HqTickError) as err:  # no resident worker set
            a.cluster_blocked(ws[0])
        assert err.value.code == abi.HQTICK_E_INVALID
        e.block_request(ws[1], 1, 1)
        a.cluster_upload(e.snapshot())  # (the snapshot's blocked triples become the resident sets)
        assert a.cluster_blocked(ws[0]) == [] and a.cluster_blocked(ws[1]) == [(1, 1)]
        a.cluster_set_blocked(ws[0], [(0, 0), (1, 0), (1, 1)])
        assert a.cluster_blocked(ws[0]) == [(0, 0), (1, 0), (1, 1)]
        assert a.cluster_enable_request(ws[0], 1, 0) == 1 and a.cluster_blocked(ws[0]) == [(0, 0), (1, 1)]
        assert a.cluster_enable_request(ws[0], 1, 0) == 0 and a.cluster_enable_request(ws[0], 7, 0) == 0 and a.cluster_blocked(ws[0]) == [(0, 0), (1, 1)]
        assert a.cluster_blocked(ws[1]) == [(1, 1)]
        for call in (lambda: a.cluster_enable_request(ws[1] + 1, 0, 0), lambda: a.cluster_blocked(ws[1] + 1)):  # an unknown worker
            with pytest.raises(HqTickError) as err:
                call()
            assert err.value.code == abi.HQTICK_E_INVALID
        assert a.cluster_enable_request(ws[0], 0, 0) == 1 and a.cluster_enable_request(ws[0], 1, 1) == 1 and a.cluster_blocked(ws[0]) == []
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 10: the audit mode
def _run_audited(a):
    _run_reject1(a)
    r = a.resident_check(abi.HQ_CHECK_ALL | abi.HQ_CHECK_STRICT)
    assert r["n_failed"] == 0, r["failed"]


def test_audit_mode_runs_the_scenario():
    """a context created with HQTICK_CHECK_RESIDENT=1 audits itself after every call that changes resident state: scenario 1 runs through, and a final strict audit
    reports nothing (a child process: the variable is read when the library creates the context)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_reject as g\n"
            "a = g._ctx()\ng._run_audited(a)\na.close()\nprint('AUDITED-OK')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HQTICK_CHECK_RESIDENT="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "AUDITED-OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- 11: the histories
class Dev(rc.DeviceSide):
    """resident_checks.DeviceSide with the two new steps and the blocked sets in every comparison"""

    def reject(self, e, triples, accepted):
        got = self.a.reject_tasks(*_cols(e, triples))
        _answer_matches(got, e, triples, accepted)
        assert self.a.assigned_last_unknown() == len(triples) - accepted

    def enable(self, e, wid, rq, v, was):
        assert self.a.cluster_enable_request(wid, rq, v) == int(was)

    def check(self, e):
        super().check(e)
        _blocked_match(self.a, e)


@pytest.mark.parametrize("form,seed", [(form, seed) for form in rj.FORMS for seed in rj.SEEDS[form]])
def test_history(form, seed):
    oracle = Oracle(abi.make_config(reserve=1, fill_max=2, **rj.lc.CFG), canonical=True)
    a = gl._ctx(form, reserve=1, fill_max=2)
    try:
        given = lambda: Oracle(abi.make_config(reserve=1, fill_max=2, **rj.lc.CFG))
        h = rj.play(rj.history(seed, form), oracle, Dev(a, form, given))
        print(f"{form} seed {seed}: {len(h.log)} steps, {h.rounds_done} rounds, " + " ".join(f"{k}={v}" for k, v in sorted(h.cov.items()) if k.startswith("HQ_REJECT")))
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- 12: one larger batch
def test_one_larger_batch_rejected_and_placed_again():
    """one tick of the 20 000-task x 64-worker workload consumed; every entry it made rejected in one shuffled call (assigned tasks with their variant, prefilled
    ones with None): the ledger is empty, the free rows are the total rows, the ready set is the uploaded one.  The next tick places nothing for a blocked pair;
    after every pair is enabled the tick is the first tick again."""
    snap = workloads.make_steady("c3p", seed=3, n_tasks=20_000, n_workers=64)
    W, R = len(snap.worker_id), snap.n_resources
    snap = dataclasses.replace(snap, assigned=[[] for _ in range(W)], worker_free=np.array(snap.worker_total, np.uint64), _keep=[])
    ids, prio, rqs = np.asarray(snap.task_id, np.uint64), np.asarray(snap.task_priority, np.uint64), np.asarray(snap.task_rq, np.uint32)
    rq_of = dict(zip(ids.tolist(), rqs.tolist())); prio_of = dict(zip(ids.tolist(), prio.tolist()))
    a = _ctx(flags=abi.HQTICK_FLAG_NO_KERNEL_TIMING)
    try:
        scn = snap.to_c(resident_workers=True)
        scn.assigned_off = None; scn.assigned_rq = None; scn.assigned_variant = None; scn.prefilled_off = None; scn.prefilled_rq = None
        a.cluster_upload(snap)
        a.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        assert len(a.graph_add_tasks(ids, prio, rqs, (np.zeros(len(ids) + 1, np.uint32), np.zeros(0, np.uint64)))) == len(ids)
        a.assigned_enable([]); a.assigned_track_prefilled([])
        tick = lambda: abi.parse_result(a.tick_raw(scn, resident=True), W, R)
        first = tick()
        a.ready_consume_last()
        wid = snap.worker_id.tolist()
        recs = [(tid, wid[w], v if k == abi.HQ_REC_ASSIGN else None) for w, rs in enumerate(first.records) for (tid, v, k) in rs]
        n_asg = sum(1 for r in recs if r[2] is not None)
        assert not first.mn and n_asg > 500 and a.assigned_count() == n_asg and a.assigned_prefilled_count() == len(recs) - n_asg and a.ready_count() == len(ids) - len(recs)
        total = np.asarray(snap.worker_total, np.uint64).reshape(W, R)
        order = np.random.default_rng(12).permutation(len(recs))
        got = a.reject_tasks([recs[k][0] for k in order], [recs[k][1] for k in order], [recs[k][2] for k in order])
        assert got["accepted"] == len(recs) and a.assigned_last_unknown() == 0
        assert got["kind"].tolist() == [K.HQ_REJECT_ASSIGNED if recs[k][2] is not None else K.HQ_REJECT_PREFILLED for k in order]
        back = sorted(r[0] for r in recs)
        assert got["requeued"] == [(x, rq_of[x], prio_of[x]) for x in back]
        assert a.assigned_count() == 0 and a.assigned_prefilled_count() == 0 and (a.assigned_free_rows() == total).all() and a.ready_count() == len(ids)
        blocked = {(w, rq_of[x], v) for (x, w, v) in recs if v is not None}
        assert {(w, q, v) for w in wid for (q, v) in a.cluster_blocked(w)} == blocked
        r = a.resident_check(abi.HQ_CHECK_ALL)
        assert r["n_failed"] == 0, r["failed"]
        second = tick()  # (never consumed: the next tick abandons it)
        placed = {(wid[w], rq_of[tid], v) for w, rs in enumerate(second.records) for (tid, v, k) in rs if k == abi.HQ_REC_ASSIGN}
        assert not placed & blocked
        for (w, q, v) in sorted(blocked):
            assert a.cluster_enable_request(w, q, v) == 1
        third = tick()
        rc.tick_equals(third, first)
        assert a.ready_remove(ids) == len(ids) and a.ready_count() == 0  # the ready set is the uploaded one: every id leaves it, nothing is left
    finally:
        a.close()
