"""hqtick_resident_check on the MI355X (include/hqtick.h; csrc/audit.hip): clean after every step of scenarios that cross the seams of the resident
structures, read-only, and every violation the public API can produce reported with its exact count and witness.  The invariants themselves are pinned on host
arrays in tests/test_audit_core.py; here the same item functions run as kernels on the state the library really keeps."""
import numpy as np
import pytest

import graph_seam_cases as S
from hyperqueue_amd import abi

pytestmark = pytest.mark.gpu

ALL, STRICT = abi.HQ_CHECK_ALL, abi.HQ_CHECK_ALL | abi.HQ_CHECK_STRICT
NOTHING = (1 << 64) - 1
PREFILLED = 3


def _clean(t, parts, where, checked=None):
    rep = t.resident_check(parts)
    assert rep["failed"] == {} and rep["n_failed"] == 0, f"{where}: {rep['failed']}"
    assert all(v == NOTHING for v in rep["first"].values()), where
    if checked is not None:
        assert rep["checked"] == checked, f"{where}: checked {rep['checked']}"
    return rep


# ---------------------------------------------------------------------------------------------- 1: a resident scenario across the seams
def _state_is(e, t):
    """what the ledger shows of every task and row against the SchedEnv mirror: worker ids, free rows, assigned (with variant), prefilled and multi-node tasks"""
    snap = e.snapshot()
    W = len(snap.worker_id)
    assert t.cluster_workers().tolist() == sorted(e.workers)
    assert (t.assigned_free_rows() == np.asarray(snap.worker_free, np.uint64).reshape(W, snap.n_resources)).all()
    ids = sorted(e.tasks)
    w, v = t.assigned_lookup(ids)
    got = {tid: (wid, var) for tid, wid, var in zip(ids, w.tolist(), v.tolist()) if wid != abi.HQ_NO_WORKER}
    want = {}
    for wid, x in e.workers.items():
        want.update({i: (wid, e._assigned_variant(i, wid)) for i in x.assigned_tasks})
        want.update({i: (wid, 0xFE) for i in x.prefilled_tasks})
        if x.mn_task is not None and x.mn_task[1]:
            want[x.mn_task[0]] = (wid, 0xFF)   # a multi-node task answers with its root
    assert got == want
    assert t.assigned_count() == sum(len(x.assigned_tasks) for x in e.workers.values())
    assert t.assigned_prefilled_count() == sum(len(x.prefilled_tasks) for x in e.workers.values())
    assert t.assigned_mn_count() == sum(1 for x in e.workers.values() if x.mn_task is not None and x.mn_task[1])


def _scenario_tick(t, snap):
    """a tick of the scenario's context: resident ready set, resident workers, the library's own Retracting table; no assigned and no prefilled CSR"""
    sc = snap.to_c(resident_workers=True)
    sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None; sc.prefilled_off = None; sc.prefilled_rq = None
    sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None
    sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
    return abi.parse_result(t.tick_raw(sc, resident=True), len(snap.worker_id), snap.n_resources)


LEDGER_FIRST_BUCKETS = 1024   # csrc/ledger.cpp: the first table; rebuilt once live entries + tombstones pass half of it


def _resident_scenario(audit: bool):
    """9 workers with 3 resources; 600 ready tasks, 200 that wait for them and 100 that wait for those (3 levels), ALL in the graph; ledger, prefilled tracking
    and clock mode on.  tick -> (audit before the consume) -> consume -> release half (and finish them in the graph) -> start prefilled -> cancel prefilled ->
    three workers join -> short tasks start and finish on one of them until the ledger's table has more entries + tombstones than half its first 1024 buckets
    (the next insert rebuilds it) -> a two-node task starts on the other two -> a worker holding single-node and prefilled tasks is lost -> the multi-node
    task's ROOT is lost (task back in the ready set, the other row single-node again) -> a higher-priority arrival dissolves the prefill sets (Retracting, back
    in their queues) -> the retracts are answered, in two halves -> tasks of 12 new requests arrive (the count rows widen past 16 slots) -> a second tick.  audit: STRICT | ALL after every step.  Returns what a twin context must reproduce bit for bit."""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import Tick
    cfg = abi.make_config(reserve=0, fill_max=2, time_limit_s=20.0)
    e = SchedEnv(cfg)
    gpu, mem = e.new_named_resource("gpus"), e.new_named_resource("mem")
    for c in (4, 4, 4, 6, 6, 2, 2, 8, 8):
        e.new_worker(WB(c).res_sum("gpus", 2).res_sum("mem", 16))
    shapes = [TB().cpus(1), TB().cpus(2), TB().cpus(1).add_resource(gpu, 1), TB().cpus(3).next_variant().cpus(1), TB().cpus(1).add_resource(mem, 4)]
    one_cpu = e.rq_id(shapes[0])
    mn_rq = e.rq_id(TB().n_nodes(2))   # the request tables the ledger is given at the upload know the multi-node request
    roots = [e.new_task(shapes[k % 5]) for k in range(600)]
    deps, level2 = {}, []
    for k in range(200):   # consumers hang on the even roots only: an odd one can be cancelled by itself
        i = e.new_task(shapes[k % 5].task_deps([roots[2 * k], roots[2 * k + 2]]))
        deps[i] = [roots[2 * k], roots[2 * k + 2]]; level2.append(i)
    for k in range(100):   # the third level
        i = e.new_task(shapes[k % 5].task_deps([level2[2 * k], level2[2 * k + 1]]))
        deps[i] = [level2[2 * k], level2[2 * k + 1]]
    has_consumers = {d for ds in deps.values() for d in ds}
    t = Tick(cfg)
    out = []

    def check(where, parts=STRICT):
        if audit:
            _clean(t, parts, where, checked=parts)

    def graph_add(ids):
        return t.graph_add_tasks(ids, [e.tasks[i].priority for i in ids], [e.tasks[i].rq for i in ids], [deps.get(i, []) for i in ids]).tolist()

    def join(cpus):
        wid = e.new_worker(WB(cpus).res_sum("gpus", 2).res_sum("mem", 16))
        s2 = e.snapshot(); k = s2.worker_id.tolist().index(wid)
        tot = np.asarray(s2.worker_total, np.uint64).reshape(len(s2.worker_id), s2.n_resources)[k:k + 1]
        t.cluster_add_workers([wid], tot, tot)
        return wid

    try:
        snap = e.snapshot()
        t.cluster_upload(snap); t.cluster_set_clock(1_000_000)
        t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        t.assigned_enable([]); t.assigned_track_prefilled([])
        assert graph_add(sorted(e.tasks)) == roots
        check("after the upload")
        # ---- the first tick, audited between the tick and its consume: the selected tasks are still in the ready set and not yet in the ledger
        r1 = _scenario_tick(t, snap)
        check("between the tick and its consume")
        t.ready_consume_last()
        e.apply(r1)
        check("after the consume")
        _state_is(e, t)
        out.append((r1.counts, r1.records, r1.new_free.tolist()))
        assert t.assigned_count() > 20 and t.assigned_prefilled_count() > 4
        # ---- half of the assigned tasks finish: out of the ledger, out of the graph, their consumers into the ready set
        running = sorted(i for i, x in e.tasks.items() if x.state in (1, 2))
        done = sorted(set(running[::2]) | {i for i in running if i in has_consumers})
        before = {i for q in e.ready.values() for i in q}
        for i in done:
            e.finish_task(i, e.tasks[i].worker)
        assert t.assigned_release(done) == len(done)
        rel, unk = t.graph_finish(done)
        assert unk == 0 and rel.tolist() == sorted({i for q in e.ready.values() for i in q} - before)
        out.append(rel.tolist())
        check("after the releases")
        # ---- prefilled tasks start
        pf = sorted(i for i, x in e.tasks.items() if x.state == PREFILLED)
        pairs = [(i, 0) for i in pf[::3]]
        for i, v in pairs:
            e.start_prefilled_task(i, v)
        assert t.assigned_start_prefilled(pairs) == len(pairs)
        check("after the starts")
        # ---- two prefilled tasks are cancelled: half done after the ledger's call (the graph still holds them, released and nowhere), whole after the graph's
        gone = [i for i in pf if e.tasks[i].state == PREFILLED and i not in has_consumers][:2]
        assert len(gone) == 2
        for i in gone:
            e.cancel_prefilled_task(i)
        assert t.assigned_unprefill(gone) == len(gone)
        if audit:
            rep = t.resident_check(STRICT)
            assert rep["failed"] == {"HQ_INV_S_RELEASED_NOWHERE": (2, min(gone))}
            _clean(t, ALL, "half of a cancel, without STRICT")
        assert t.graph_remove(np.asarray(gone, np.uint64)).tolist() == sorted(gone)
        check("after the cancels")
        # ---- three workers join
        wa, wb, wc = join(4), join(4), join(4)
        check("after the workers joined")
        # ---- short tasks start and finish on the first of them, four at a time (its 4 cpus), between two ticks: every release leaves a tombstone, and the
        # ---- table of 1024 buckets is due for a rebuild once entries + tombstones pass 512.  (They never enter the graph: audited without STRICT while they run.)
        churned = 0
        for k in range(140):
            ids = [(1 << 40) + 4 * k + j for j in range(4)]
            assert t.assigned_add([(i, wa, one_cpu, 0, 0) for i in ids]) == 4
            if k == 70:
                check("short tasks running", ALL)
            assert t.assigned_release(ids) == 4
            churned += 4
        assert churned + t.assigned_count() + t.assigned_prefilled_count() > LEDGER_FIRST_BUCKETS // 2
        check("after the short tasks")
        # ---- a two-node task arrives and starts on the other two (root first): the insert rebuilds the table, every key is probed for in the new one
        mn = e.new_task(TB().n_nodes(2))
        assert e.tasks[mn].rq == mn_rq and graph_add([mn]) == [mn]
        check("a multi-node task is ready")
        assert t.ready_remove([mn]) == 1 and t.assigned_add_mn([(mn, mn_rq, e.tasks[mn].priority, [wb, wc])]) == 1
        e.start_task_mn(mn, [wb, wc])
        check("after the multi-node task started")
        assert t.assigned_mn_workers(mn) == [wb, wc]
        # ---- a worker that holds single-node and prefilled tasks is lost: its tasks go back into the resident ready set
        lost = next(w for w, x in sorted(e.workers.items()) if x.assigned_tasks and x.prefilled_tasks)
        back = sorted(set(e.workers[lost].assigned_tasks) | set(e.workers[lost].prefilled_tasks))
        assert e.remove_worker(lost) == [] and t.cluster_remove_workers([lost]) == []
        assert [x[0] for x in t.cluster_last_requeued()] == back
        check("after a worker was lost")
        _state_is(e, t)
        # ---- the multi-node task's root is lost: the task is back in its queue, the other worker is free again
        assert e.remove_worker(wb) == [] and t.cluster_remove_workers([wb]) == []
        assert [x[0] for x in t.cluster_last_requeued()] == [mn] and t.assigned_mn_count() == 0
        check("after the multi-node root was lost")
        _state_is(e, t)
        e.cancel_task(mn)   # ... and is cancelled, so that the second tick is about single-node tasks
        assert t.ready_remove([mn]) == 1 and t.graph_remove(np.asarray([mn], np.uint64)).tolist() == [mn]
        check("after the multi-node task was cancelled")
        # ---- a higher-priority arrival dissolves every prefill set: the tasks are Retracting{worker}, back in their queues (process_retracted, reactor.rs:34-62)
        n_msgs = len(e.retract_messages)
        hi = e.new_task(TB().cpus(1).user_priority(1))
        msgs = sorted(e.retract_messages[n_msgs:], key=lambda m: m[1])
        assert len(msgs) >= 4
        ids = [x for (_, x) in msgs]
        assert t.assigned_unprefill(ids) == len(ids) and t.assigned_prefilled_count() == 0
        t.retracting_add(ids, [w for (w, _) in msgs])
        t.ready_compact()
        t.ready_add(np.asarray(ids, np.uint64), np.asarray([e.tasks[x].priority for x in ids], np.uint64), np.asarray([e.tasks[x].rq for x in ids], np.uint32))
        assert graph_add([hi]) == [hi]
        check("after the prefill sets were dissolved")
        # ---- the workers answer the retracts, half of them first: those tasks are ordinary waiting tasks of their queues again.  (All are answered before the
        # ---- next tick: one that finds a Retracting task where it would prefill is refused, as the reference asserts there, mapping.rs:221.)
        for part in (msgs[::2], msgs[1::2]):
            for (w, x) in part:
                e.retract_response(w, [x])
                assert t.retract_response(w, [x]) == []
            check("after retract responses")
        assert t.retracting_count() == 0
        # ---- tasks of 12 new requests: 19 variant slots, the count rows widen; then the second tick
        new = [e.new_task(TB().cpus(1).add_resource(mem, k + 1)) for k in range(12) for _ in range(3)]
        assert graph_add(new) == new
        check("after the arrivals")
        snap = e.snapshot()
        r2 = _scenario_tick(t, snap)
        check("between the second tick and its consume")
        t.ready_consume_last()
        e.apply(r2)
        check("after the second tick")
        _state_is(e, t)
        assert t.retracting_count() == sum(1 for x in e.tasks.values() if x.state == 4)
        out.append((r2.counts, r2.records, r2.new_free.tolist(), r2.redirects))
        st = t.graph_stats(); st.pop("last_kernel_us")
        out += [t.assigned_free_rows().tolist(), t.ready_count(), st, t.assigned_count(), t.assigned_prefilled_count()]
        return out
    finally:
        t.close()


def test_clean_after_every_step_and_a_twin_that_never_audits_ends_the_same():
    """the audit after every step (and between both ticks and their consumes, which go on to work), then the same scenario on a context that never audits: tick
    results, free rows, ready count and graph statistics are identical -- the audit changed no resident byte and abandoned nothing"""
    audited = _resident_scenario(True)
    plain = _resident_scenario(False)
    assert audited == plain


from resident_checks import sanity_check_free as _sanity_check_free  # noqa: E402  (Worker::sanity_check on the mirror)


class _AuditHost:
    """test_gpu_assigned_prefill's ledger host, auditing after every event it checks"""

    def __new__(cls, cfg):
        from test_gpu_assigned_prefill import _Host

        class H(_Host):
            audits = overcommitted = 0
            ready_resident = False

            # _Host uploads a ready set before a worker is lost and keeps it current to the end of that round; the next round's arrivals reach only the snapshot.
            # A host with a resident set sends them: here the set is uploaded again at the start of the round (the tick by hqtick_run then drops it)
            def before_loss(self, snap):
                super().before_loss(snap); self.ready_resident = True

            def upload(self, snap):
                super().upload(snap)
                if self.ready_resident:
                    self.a.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)

            def tick(self, snap, want):
                super().tick(snap, want); self.ready_resident = False

            def check(self, e):
                super().check(e)
                if self.uploaded:
                    bad = _sanity_check_free(e)
                    rep = self.a.resident_check(ALL)
                    assert rep["failed"] == ({"HQ_INV_LEDGER_FREE": (len(bad), min(bad))} if bad else {}), f"audit {H.audits}"
                    H.audits += 1; H.overcommitted += bool(bad)
        h = H(cfg)
        cls.last = H
        return h


@pytest.mark.parametrize("seed", [0, 3])
def test_the_prefilled_scenarios_stay_clean(seed):
    """the random scenarios of test_gpu_assigned_prefill.py (ticks by hqtick_run, starts, releases, cancels, rejects, dissolved prefill sets, retract responses with
    redirects, joins, lost workers whose tasks go back into a resident ready set): hqtick_resident_check(HQ_CHECK_ALL) after every event.  Clean, but for the
    free rows of workers the generator over-committed: there the audit reports exactly what Worker::sanity_check finds on the mirror"""
    from test_gpu_assigned_prefill import _scenario

    st = _scenario(seed, host_cls=_AuditHost)
    assert st["ticks"] >= 2 and _AuditHost.last.audits >= 10
    if seed == 0:   # this seed starts prefilled tasks on full workers: the comparison with Worker::sanity_check was about real findings
        assert _AuditHost.last.overcommitted >= 1


# ---------------------------------------------------------------------------------------------- 2: violations the public API can produce
def _small_ctx():
    """2 workers of 4 cpus (ids 50, 51); requests 0 = 1 cpu, 1 = all cpus, 2 = 2 cpus | 1 cpu; ledger and tracking on; an empty resident ready set"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB
    from hyperqueue_amd.tick import Tick

    cfg = abi.make_config(reserve=0, fill_max=2, time_limit_s=20.0)
    e = SchedEnv(cfg)
    e.new_workers_cpus([4, 4])
    assert [e.rq_id(b) for b in (TB().cpus(1), TB().cpus_all(), TB().cpus(2).next_variant().cpus(1))] == [0, 1, 2]
    t = Tick(cfg)
    t.cluster_upload(e.snapshot())
    t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    t.assigned_enable([]); t.assigned_track_prefilled([])
    return e, t


def _ready_add(t, ids, rq=0):
    ids = np.asarray(ids, np.uint64)
    t.ready_add(ids, np.zeros(len(ids), np.uint64), np.full(len(ids), rq, np.uint32))


def test_a_free_value_overwritten_by_update_workers():
    e, t = _small_ctx()
    try:
        assert t.assigned_add([(10, 50, 0, 0, 0), (11, 51, 0, 0, 0), (12, 51, 2, 1, 0)]) == 3
        _clean(t, ALL, "three running tasks", checked=abi.HQ_CHECK_READY | abi.HQ_CHECK_LEDGER | abi.HQ_CHECK_CROSS)
        rows = t.assigned_free_rows().copy()
        assert rows.tolist() == [[30_000], [20_000]]
        rows[1, 0] += 1
        t.cluster_update_workers([1], rows[1:2])
        rep = t.resident_check(ALL)
        assert rep["failed"] == {"HQ_INV_LEDGER_FREE": (1, 51 << 32 | 0)} and rep["n_failed"] == 1
        assert rep["kernel_us"] > 0
        rows[1, 0] -= 1
        t.cluster_update_workers([1], rows[1:2])
        _clean(t, ALL, "corrected")
    finally:
        t.close()


@pytest.mark.parametrize("order", ["B_then_A", "A_then_B"])
def test_a_release_batch_of_an_all_and_an_amount_entry(order):
    """A = 1 cpu (AMOUNT), B = all cpus (ALL) on worker 50.  include/hqtick.h: "B, then A" leaves total + amount(A) in the free row -- reported; "A, then B" the total"""
    e, t = _small_ctx()
    try:
        assert t.assigned_add([(20, 50, 0, 0, 0), (21, 50, 1, 0, 0)]) == 2
        assert t.assigned_free_rows().tolist() == [[0], [40_000]]
        _clean(t, ALL, "both running")
        assert t.assigned_release([21, 20] if order == "B_then_A" else [20, 21]) == 2
        rep = t.resident_check(ALL)
        if order == "B_then_A":
            assert t.assigned_free_rows().tolist() == [[50_000], [40_000]]
            assert rep["failed"] == {"HQ_INV_LEDGER_FREE": (1, 50 << 32 | 0)}
        else:
            assert t.assigned_free_rows().tolist() == [[40_000], [40_000]]
            assert rep["failed"] == {}
    finally:
        t.close()


def test_ready_adds_that_break_the_cross_invariants():
    e, t = _small_ctx()
    try:
        # the graph holds 1, 2 and 3 (which waits for 1); 1 and 2 are ready; 1 is handed out and runs on worker 50
        assert t.graph_add_tasks([1, 2, 3], [0, 0, 0], [0, 0, 0], [[], [], [1]]).tolist() == [1, 2]
        assert t.ready_remove([1]) == 1 and t.assigned_add([(1, 50, 0, 0, 0)]) == 1
        _clean(t, STRICT, "consistent", checked=STRICT)
        # an id the ledger holds
        t.ready_compact()   # (the tombstone of 1 goes: the id may come back)
        _ready_add(t, [1])
        assert t.resident_check(STRICT)["failed"] == {"HQ_INV_X_READY_ASSIGNED": (1, 1)}
        assert t.ready_remove([1]) == 1
        t.ready_compact()
        # an id the graph holds with a non-zero counter
        _ready_add(t, [3])
        assert t.resident_check(STRICT)["failed"] == {"HQ_INV_X_READY_WAITING": (1, 3)}
        assert t.ready_remove([3]) == 1
        # an id unknown to the graph: clean for a host that keeps only some tasks there, reported under STRICT
        _ready_add(t, [7, 9])
        _clean(t, ALL, "unknown ids without STRICT")
        assert t.resident_check(STRICT)["failed"] == {"HQ_INV_S_READY_UNKNOWN": (2, 7)}
        assert t.ready_remove([7, 9]) == 2
        # a released task that leaves the ready set and goes nowhere
        assert t.ready_remove([2]) == 1
        _clean(t, ALL, "a task nobody took, without STRICT")
        assert t.resident_check(STRICT)["failed"] == {"HQ_INV_S_RELEASED_NOWHERE": (1, 2)}
        t.ready_compact()
        _ready_add(t, [2])
        _clean(t, STRICT, "back")
        # a Retracting task that is not in its queue
        t.retracting_add([2, 5], [51, 51])
        assert t.resident_check(STRICT)["failed"] == {"HQ_INV_X_RETRACTING": (1, 5)}
        # a ledger id the graph holds with a non-zero counter
        assert t.assigned_add([(3, 51, 0, 0, 0)]) == 1
        rep = t.resident_check(STRICT)["failed"]
        assert rep == {"HQ_INV_X_RETRACTING": (1, 5), "HQ_INV_S_ASSIGNED_WAITING": (1, 3)}
    finally:
        t.close()


def test_multi_node_rows_and_their_entry():
    """two multi-node tasks over four of six workers: clean; after the release of one its rows are single-node rows again, still clean"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB
    from hyperqueue_amd.tick import Tick

    cfg = abi.make_config(time_limit_s=20.0)
    e = SchedEnv(cfg)
    e.new_workers_cpus([4] * 6)
    assert [e.rq_id(b) for b in (TB().cpus(1), TB().n_nodes(2))] == [0, 1]
    t = Tick(cfg)
    try:
        t.cluster_upload(e.snapshot()); t.assigned_enable([])
        assert t.assigned_add_mn([(100, 1, 0, [52, 50]), (101, 1, 0, [53, 55])]) == 2 and t.assigned_add([(5, 51, 0, 0, 0)]) == 1
        _clean(t, ALL, "two multi-node tasks", checked=abi.HQ_CHECK_LEDGER)
        assert t.assigned_release([100]) == 1
        _clean(t, ALL, "one released")
        assert t.assigned_mn_count() == 1 and t.assigned_count() == 1
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------- 3: parts that are not resident are skipped
def test_absent_structures_are_skipped_and_bad_arguments_refused():
    import ctypes as C

    from hyperqueue_amd.tick import HqTickError, Tick

    t = Tick(abi.make_config())
    try:
        rep = _clean(t, STRICT, "nothing resident", checked=0)
        assert rep["kernel_us"] == 0.0
        ids = np.arange(10, 2000, 3, dtype=np.uint64)
        t.upload_ready(ids, np.zeros(len(ids), np.uint64), np.zeros(len(ids), np.uint32))
        assert t.ready_remove(ids[5:700:7]) == len(ids[5:700:7])
        rep = _clean(t, STRICT, "a ready set alone", checked=abi.HQ_CHECK_READY)
        assert all(rep["count"][n] == 0 and rep["first"][n] == NOTHING for n in abi.HQ_INV_NAMES if "LEDGER" in n)
        with pytest.raises(HqTickError) as err:
            t.resident_check(32)
        assert err.value.code == abi.HQTICK_E_INVALID
        t._lib.hqtick_resident_check.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        assert t._lib.hqtick_resident_check(t._ctx, 1, None) == abi.HQTICK_E_INVALID
        assert t._lib.hqtick_resident_check(None, 1, None) == abi.HQTICK_E_INVALID
        _clean(t, ALL, "after the refusals", checked=abi.HQ_CHECK_READY)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------- 4: the graph's seam histories, audited after every step
class _Audited:
    """a Tick whose mutating graph / ready-set methods end with the audit of the graph, the ready set and what must hold between them"""
    PARTS = abi.HQ_CHECK_GRAPH | abi.HQ_CHECK_READY | abi.HQ_CHECK_CROSS
    MUTATING = ("graph_add_tasks", "graph_finish", "graph_remove", "graph_blevel", "ready_remove", "ready_add", "upload_ready", "tick")

    def __init__(self, t):
        self._t, self.audits, self.findings = t, 0, []

    def __getattr__(self, name):
        f = getattr(self._t, name)
        if name not in self.MUTATING:
            return f

        def call(*a, **k):
            try:
                return f(*a, **k)
            finally:   # (also after a call the graph refuses: the history goes on from the state it left)
                rep = self._t.resident_check(self.PARTS)
                self.audits += 1
                if rep["failed"]:
                    self.findings.append((name, self.audits, rep["failed"]))
        return call


SEAMS = [("mixed_chain", ()), ("hash_cluster", S.MIN_HASH_CAP - 1), ("hash_cluster", 0), ("edge_pool", "exact"), ("edge_pool", "over"), ("bfs_diamond", ()),
         ("run_lengths", "gate_first")]


@pytest.mark.parametrize("family,arg", SEAMS, ids=[f"{f}-{a}" if a != () else f for f, a in SEAMS])
def test_the_seam_histories_stay_clean(family, arg):
    """tests/graph_seam_cases.py, unchanged: wherever the runner's own comparison with the graph oracle holds, the audit is clean"""
    from hyperqueue_amd.tick import Tick

    t = Tick(abi.make_config(time_limit_s=20.0))
    try:
        t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        a = _Audited(t)
        S.run(a, S.build(family, arg))
        assert a.audits >= 3
        assert a.findings == []
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------- 5: HQTICK_CHECK_RESIDENT=1
def test_the_debug_flag_audits_behind_every_state_changing_call():
    """with HQTICK_CHECK_RESIDENT=1 at hqtick_create the scenario above runs without an error (every delta, consume and tick ends with the audit of READY | LEDGER |
    GRAPH), and a free value overwritten through hqtick_cluster_update_workers -- a correction call, which stays asynchronous and is not audited itself -- makes the
    NEXT state-changing call fail with HQTICK_E_INVALID and a text that names the invariant and the witness"""
    from hyperqueue_amd.tick import HqTickError
    from test_gpu_assigned_prefill import _Env

    with _Env(HQTICK_CHECK_RESIDENT="1"):
        plain = _resident_scenario(False)
        e, t = _small_ctx()
    try:
        assert plain[-2] > 0   # (the scenario's own last figures: assigned entries at its end)
        assert t.assigned_add([(10, 50, 0, 0, 0), (11, 51, 0, 0, 0)]) == 2
        rows = t.assigned_free_rows().copy()
        rows[1, 0] += 1
        t.cluster_update_workers([1], rows[1:2])
        with pytest.raises(HqTickError) as err:
            t.assigned_add([(12, 51, 0, 0, 0)])
        assert err.value.code == abi.HQTICK_E_INVALID
        assert "HQ_INV_LEDGER_FREE" in str(err.value) and str(51 << 32 | 0) in str(err.value)
        assert t.assigned_count() == 3   # what the call did stays done
    finally:
        t.close()
