"""Clock mode of the resident worker set (hqtick_cluster_set_clock): the termination times stay with the worker set, a tick takes only the clock,
and k_clock_rows turns `deadline - clock` into the canonical remaining-lifetime column.  Every clock-mode tick equals the tick of a context that is given the true
lifetimes (per-tick packing, or the row-delta protocol), workers that differ only in their deadlines stay ONE group of equal rows, a ledger host never calls
hqtick_cluster_update_workers, and a context that never sets the clock launches nothing new.  HQTICK_CHECK_CLUSTER=1 throughout: every tick compares the column in
HBM with the host mirror."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads

pytestmark = pytest.mark.gpu

S = 1_000_000_000
NO_LIMIT = abi.HQ_NO_TIME_LIMIT
CHUNK = 256  # thresholds k_clock_rows stages in LDS at a time (csrc/clock_core.h)


def _tick(measure=False, flags=0, **env):
    from hyperqueue_amd.tick import Tick

    env.setdefault("HQTICK_CHECK_CLUSTER", 1)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Tick(abi.make_config(time_limit_s=20.0, flags=flags), measure=measure)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(a, b):
    assert a.status == b.status and a.batches == b.batches
    assert a.counts == b.counts and a.records == b.records and a.retracts == b.retracts
    assert (a.new_free == b.new_free).all()


def _variant(entries, min_time_s=0):
    v = workloads._variant(entries)
    v["min_time_ns"] = int(min_time_s * S)
    return v


def _snap(ids, total, term, now, requests, tasks, free=None):
    """a snapshot of idle workers `ids` with termination times `term` (NO_LIMIT: none) seen at `now`: the TRUE remaining lifetimes"""
    ids = np.asarray(ids, np.uint32); n = len(ids)
    total = np.asarray(total, np.uint64).reshape(n, -1)
    term = np.asarray(term, np.int64)
    rem = np.where(term == NO_LIMIT, NO_LIMIT, term - np.int64(now)).astype(np.int64)
    tid, prio, rq = tasks
    return abi.Snapshot(n_resources=total.shape[1], worker_id=ids, worker_total=total, worker_free=total.copy() if free is None else np.asarray(free, np.uint64).reshape(n, -1),
                        worker_remaining_ns=rem, worker_min_utilization=np.zeros(n, np.float32), worker_flags=np.full(n, abi.HQ_WORKER_SN, np.uint8),
                        worker_group=np.zeros(n, np.uint32), n_groups=1, blocked=[], assigned=[[] for _ in range(n)], prefilled=[[] for _ in range(n)],
                        requests=requests, task_id=tid, task_priority=prio, task_rq=rq)


def _tasks(n, rqs, seed):
    ids = (np.uint64(1) << np.uint64(32)) | np.arange(1, n + 1, dtype=np.uint64)
    rq = np.asarray(rqs, np.uint32)[np.random.default_rng(seed).integers(0, len(rqs), size=n)]
    return ids, np.full(n, workloads.priority_from_user(0), np.uint64), rq


REQ3 = [[_variant([(0, 1)], 0)], [_variant([(0, 4)], 10)], [_variant([(0, 2), (1, 1)], 100)], [_variant([(0, 8)], 100), _variant([(0, 2)], 10)], [_variant([(0, 1), (2, 1)], 0)]]


def test_parity_across_thresholds():
    """48 workers with staggered termination times, requests with min_time 0 / 10 s / 100 s (one with two variants of different min_time), eight ticks between which
    the clock jumps so that every tick some workers cross a threshold and some pass their termination: the clock-mode context, driven by set_clock alone, equals
    per-tick packing with the true lifetimes and the canonical oracle."""
    from oracle.oracle import Oracle

    W, now0 = 48, 1000 * S
    ids = np.arange(1, W + 1)
    total = np.tile(np.asarray([16, 2, 64], np.uint64) * np.uint64(workloads.FR), (W, 1))
    term = now0 + (np.arange(W, dtype=np.int64) * 5 - 20) * S + np.arange(W, dtype=np.int64) * 1017  # 5 s apart (and a little): -20 s .. 215 s
    term[::7] = NO_LIMIT
    tasks = _tasks(20_000, [0, 1, 2, 3, 4], seed=1)
    plain, res, o = _tick(), _tick(), Oracle(abi.make_config(time_limit_s=20.0), canonical=True)
    try:
        res.cluster_upload(_snap(ids, total, term, now0, REQ3, tasks))
        seen = set()
        for k, jump in enumerate([0, 7, 19, 33, 58, 90, 131, 177]):
            now = now0 + jump * S
            snap = _snap(ids, total, term, now, REQ3, tasks)
            res.cluster_set_clock(now)
            got = res.tick(snap, resident_workers=True)
            _same(got, plain.tick(snap))
            _same(got, o.tick(snap))
            assert (res.cluster_deadlines() == term).all()
            rem = snap.worker_remaining_ns[term != NO_LIMIT]
            cls = tuple(int(((rem >= lo) & (rem < hi)).sum()) for lo, hi in ((-1 << 62, 0), (0, 10 * S), (10 * S, 100 * S), (100 * S, 1 << 62)))
            assert cls not in seen and (k == 0 or cls[0] > last[0]), (k, cls)  # workers crossed thresholds and passed their termination since the last tick
            seen.add(cls); last = cls
        assert res.cluster_last_row_groups() < plain.cluster_last_row_groups()
    finally:
        plain.close(); res.close()


@pytest.mark.parametrize("n_filler", [0, CHUNK + 1 - 6])
def test_geometry(n_filler):
    """300 workers: the second workgroup of k_clock_rows is partly filled, and only rows 0, 63, 64, 255, 256 and 299 — the edges of wavefronts and workgroups — have a
    time limit, each in another time class.  n_filler > 0: the request table is one variant longer than the chunk of thresholds the kernel stages in LDS, and the
    threshold that decides the last class sits in the second chunk."""
    W, now = 300, 50 * S
    rows = [0, 63, 64, 255, 256, 299]
    term = np.full(W, NO_LIMIT, np.int64)
    term[rows] = now + np.asarray([-3, 5, 15, 25, 45, 55], np.int64) * S  # past | 0 only | 10 | 20 | 40 | 50 s
    reqs = [[_variant([(0, 1)], 10 * k)] for k in range(5)] + [[_variant([(0, 1)], 1000 + i)] for i in range(n_filler)] + [[_variant([(0, 1)], 50)]]
    assert sum(len(r) for r in reqs) == (6 if not n_filler else CHUNK + 1)
    used = [0, 1, 2, 3, 4, len(reqs) - 1]
    ids = np.arange(10, 10 + W)
    total = np.full((W, 1), 2 * workloads.FR, np.uint64)
    tasks = _tasks(3_000, used, seed=2)
    plain, res = _tick(), _tick()
    try:
        res.cluster_upload(_snap(ids, total, term, now - 7 * S, reqs, tasks))
        res.cluster_set_clock(now - 7 * S)
        res.cluster_set_clock(now)
        snap = _snap(ids, total, term, now, reqs, tasks)
        got, want = res.tick(snap, resident_workers=True), plain.tick(snap)
        _same(got, want)
        assert (res.cluster_deadlines() == term).all()
        # what each row may run is what its time class allows: the tasks of request k need 10 k seconds (the last request 50)
        need = {rq: v[0]["min_time_ns"] for rq, v in enumerate(reqs)}
        rq_of = dict(zip(tasks[0].tolist(), tasks[2].tolist()))
        for w, left in zip(rows, [-3, 5, 15, 25, 45, 55]):
            ran = {need[rq_of[t]] for (t, _, kind) in got.records[w] if kind == abi.HQ_REC_ASSIGN}
            assert all(x <= left * S for x in ran) and (left >= 0 or not ran), (w, left, sorted(ran))
        assert res.cluster_last_row_groups() == 7  # six time classes and the workers without a limit
    finally:
        plain.close(); res.close()


def test_ledger_host_never_sends_rows():
    """Assignment ledger on, time-limited workers: context A keeps ledger and clock — it is told releases, starts and the time, and never calls
    hqtick_cluster_update_workers; context B runs the row-delta protocol (all rows with free resources and true lifetimes before every tick, the assigned CSR in the
    snapshot).  Every tick of A equals B's and A's free rows equal the reference state's after every event."""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from hyperqueue_amd.tick import Tick

    rng = np.random.default_rng(77)
    cfg = abi.make_config(time_limit_s=20.0)
    e = SchedEnv(cfg)
    e.now_ns = 500 * S
    os.environ["HQTICK_CHECK_CLUSTER"] = "1"
    try:
        a, b = Tick(cfg), Tick(cfg)
    finally:
        os.environ.pop("HQTICK_CHECK_CLUSTER", None)
    a.cluster_update_workers = None  # the ledger host has no free rows to send: any call would raise
    shapes = [TB().cpus(1), TB().cpus(2).time_request(10), TB().cpus(1).time_request(100), TB().cpus(3).time_request(100).next_variant().cpus(1).time_request(10), TB().cpus(0.5)]
    for i, lim in enumerate([12, 25, 40, 70, 110, 130, 400, None]):
        e.new_worker(WB(4 + i % 3) if lim is None else WB(4 + i % 3).time_limit_s(lim + 0.001 * i))
    n_msgs, n_ticks, n_started, crossed = 0, 0, 0, set()

    def free_of(snap):
        return np.asarray(snap.worker_free, np.uint64).reshape(len(snap.worker_id), snap.n_resources)

    try:
        for round_ in range(8):
            for k in range(int(rng.integers(2, 8)) if round_ else 24):
                e.new_task(shapes[k if not round_ and k < len(shapes) else int(rng.integers(0, len(shapes)))])  # (every request class exists from the first snapshot on)
            new_msgs = e.retract_messages[n_msgs:]; n_msgs = len(e.retract_messages)
            snap = dataclasses.replace(e.snapshot(), worker_map_rank=None, _keep=[])
            W = len(snap.worker_id)
            if round_ == 0:
                a.cluster_upload(snap); a.assigned_enable([])
                b.cluster_upload(snap)
            else:
                b.cluster_update_workers(np.arange(W), free_of(snap), snap.worker_remaining_ns)
            if new_msgs:
                a.retracting_add([t for (_, t) in new_msgs], [w for (w, _) in new_msgs])
            a.cluster_set_clock(e.now_ns)
            want = b.tick(snap, resident_workers=True)
            sc = snap.to_c(resident_workers=True)
            sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
            sc.n_retracting = abi.HQ_RETRACTING_RESIDENT; sc.retracting_task = None; sc.retracting_worker = None; sc.retracting_redirect_worker = None; sc.retracting_redirect_variant = None
            got = abi.parse_result(a.tick_raw(sc), W, snap.n_resources)
            _same(got, want)
            assert got.redirects == want.redirects
            e.apply(want); n_ticks += 1
            assert (a.assigned_free_rows() == free_of(e.snapshot())).all()
            crossed.add(tuple(int(x) for x in np.searchsorted([0, 10 * S, 100 * S], snap.worker_remaining_ns[:-1], side="right")))
            for wid, w in sorted(e.workers.items()):  # tasks that start outside a tick (a host that assigned them itself): the ledger is told, no row is sent
                if w.free[0] >= workloads.FR // 2 and rng.random() < 0.4:
                    tid = e.new_task_running(shapes[4], wid)
                    t = e.tasks[tid]
                    assert a.assigned_add([(tid, wid, t.rq, 0, t.priority)]) == 1
                    n_started += 1
            assert (a.assigned_free_rows() == free_of(e.snapshot())).all()
            done = [t for t in sorted(e.tasks.values(), key=lambda t: t.id) if t.state in (1, 2) and rng.random() < 0.4]
            for t in done:
                e.finish_task(t.id, t.worker)
            assert a.assigned_release([t.id for t in done]) == len(done)
            assert (a.assigned_free_rows() == free_of(e.snapshot())).all()
            e.now_ns += int(rng.integers(9, 21)) * S  # time passes: only the clock tells A
        assert n_ticks == 8 and n_started >= 3 and len(crossed) >= 5, (n_started, crossed)  # the workers' time classes kept changing
    finally:
        a.close(); b.close()


def test_deltas_in_clock_mode():
    """workers join, leave and are corrected in clock mode: the deadlines follow their rows, a remaining lifetime given to an old call is one at the current clock"""
    W, now = 12, 300 * S
    ids = list(range(1, W + 1))
    tot_row = np.asarray([8, 1, 32], np.uint64) * np.uint64(workloads.FR)
    term = [now + k * 11 * S for k in range(W)]  # 0 .. 121 s
    term[4] = NO_LIMIT
    tasks = _tasks(6_000, [0, 1, 2, 3, 4], seed=3)
    plain, res = _tick(), _tick()

    def check():
        snap = _snap(ids, np.tile(tot_row, (len(ids), 1)), term, now, REQ3, tasks)
        assert res.cluster_workers().tolist() == ids and res.cluster_deadlines().tolist() == term
        _same(res.tick(snap, resident_workers=True), plain.tick(snap))

    try:
        res.cluster_upload(_snap(ids, np.tile(tot_row, (W, 1)), term, now, REQ3, tasks))
        res.cluster_set_clock(now)
        check()
        now += 6 * S; res.cluster_set_clock(now)
        res.cluster_add_workers([40, 41], np.stack([tot_row, tot_row]), remaining_ns=[25 * S, NO_LIMIT])  # 25 s from NOW
        ids += [40, 41]; term += [now + 25 * S, NO_LIMIT]
        check()
        res.cluster_remove_workers([ids[5], ids[-1]])  # a middle and the last worker
        del ids[5], term[5]; del ids[-1], term[-1]
        check()
        res.cluster_update_workers([3], tot_row.reshape(1, -1), remaining_ns=[142 * S])  # a correction: row 3 has 142 s left at the current clock
        term[3] = now + 142 * S
        check()
        now -= 40 * S; res.cluster_set_clock(now)  # the clock may move back: lifetimes grow again
        check()
        now += 400 * S; res.cluster_set_clock(now)  # ... and everyone with a limit is past it
        check()
    finally:
        plain.close(); res.close()


def test_new_request_class_re_canonicalises_in_the_same_tick():
    """a snapshot brings a request class whose min_time (50 s) lies between two thresholds of the table in HBM: the workers between 10 s and 100 s split at once"""
    now = 0
    left = [5, 30, 45, 55, 70, 150, 99, 51, 49, 12]
    ids, term = list(range(1, len(left) + 1)), [now + x * S for x in left]
    total = np.tile(np.asarray([8, 1, 32], np.uint64) * np.uint64(workloads.FR), (len(ids), 1))
    plain, res = _tick(), _tick()
    try:
        old = _snap(ids, total, term, now, REQ3, _tasks(4_000, [0, 1, 2, 3, 4], seed=4))
        res.cluster_upload(old); res.cluster_set_clock(now)
        _same(res.tick(old, resident_workers=True), plain.tick(old))
        assert res.cluster_last_row_groups() == 3
        new = _snap(ids, total, term, now, REQ3 + [[_variant([(0, 1)], 50)]], _tasks(4_000, [5], seed=5))  # (only tasks of the new class are ready)
        for _ in range(2):  # that tick and the next
            got = res.tick(new, resident_workers=True)
            _same(got, plain.tick(new))
            assert res.cluster_last_row_groups() == 4
            rq_of = dict(zip(new.task_id.tolist(), new.task_rq.tolist()))
            for w, x in enumerate(left):  # 50 s of lifetime are needed to start a task of the new class, and there are far more tasks than room
                assert any(rq_of[t] == 5 for (t, _, kind) in got.records[w] if kind == abi.HQ_REC_ASSIGN) == (x >= 50), (w, x)
        _same(res.tick(old, resident_workers=True), plain.tick(old))  # and back
        assert res.cluster_last_row_groups() == 3
    finally:
        plain.close(); res.close()


def test_equal_workers_stay_one_group():
    """64 identical idle workers with 64 distinct deadlines beyond the largest threshold: ONE group of equal rows in clock mode, 64 on the row-delta protocol with
    the true lifetimes — and the same result.  With half of the deadlines between two thresholds: two groups."""
    W, now = 64, 10_000 * S
    ids = np.arange(1, W + 1)
    total = np.tile(np.asarray([8, 1, 32], np.uint64) * np.uint64(workloads.FR), (W, 1))
    tasks = _tasks(8_000, [0, 1, 2, 3, 4], seed=6)
    term = now + 200 * S + np.arange(W, dtype=np.int64) * 1_000  # connected microseconds apart
    rows, res = _tick(), _tick()
    try:
        snap = _snap(ids, total, term, now, REQ3, tasks)
        rows.cluster_upload(snap); res.cluster_upload(snap)
        res.cluster_set_clock(now)
        a, b = res.tick(snap, resident_workers=True), rows.tick(snap, resident_workers=True)
        _same(a, b)
        assert res.cluster_last_row_groups() == 1 and rows.cluster_last_row_groups() == 64
        now += 3 * S
        snap = _snap(ids, total, term, now, REQ3, tasks)
        res.cluster_set_clock(now)
        rows.cluster_update_workers(np.arange(W), total, snap.worker_remaining_ns)  # all W rows again, for the time alone
        _same(res.tick(snap, resident_workers=True), rows.tick(snap, resident_workers=True))
        assert res.cluster_last_row_groups() == 1 and rows.cluster_last_row_groups() == 64
        term2 = term.copy(); term2[::2] -= 150 * S  # every other worker: between 10 s and 100 s
        snap = _snap(ids, total, term2, now, REQ3, tasks)
        res.cluster_upload(snap); rows.cluster_upload(snap)
        res.cluster_set_clock(now)
        _same(res.tick(snap, resident_workers=True), rows.tick(snap, resident_workers=True))
        assert res.cluster_last_row_groups() == 2 and rows.cluster_last_row_groups() == 64
    finally:
        rows.close(); res.close()


def test_refusals_change_nothing():
    from hyperqueue_amd.tick import HqTickError

    now = 77 * S
    ids, term = [1, 2, 3, 4], [now + 5 * S, now + 50 * S, NO_LIMIT, now + 500 * S]
    total = np.tile(np.asarray([8, 1, 32], np.uint64) * np.uint64(workloads.FR), (4, 1))
    tasks = _tasks(2_000, [0, 1, 2, 3, 4], seed=7)
    snap = _snap(ids, total, term, now, REQ3, tasks)
    plain, t, sh, led = _tick(), _tick(), _tick(), _tick()
    try:
        with pytest.raises(HqTickError) as err:  # no resident worker set
            t.cluster_set_clock(now)
        assert err.value.code == abi.HQTICK_E_INVALID
        with pytest.raises(HqTickError) as err:
            t.cluster_deadlines()
        assert err.value.code == abi.HQTICK_E_INVALID
        t.cluster_upload(snap)
        with pytest.raises(HqTickError):  # a resident set outside clock mode has no deadlines
            t.cluster_deadlines()
        _same(t.tick(snap), plain.tick(snap))  # outside clock mode a snapshot may bring its worker arrays
        t.cluster_set_clock(now)
        want = plain.tick(snap)
        with pytest.raises(HqTickError) as err:  # a clock-mode tick that brings worker arrays: two truths
            t.tick(snap)
        assert err.value.code == abi.HQTICK_E_INVALID and "clock mode" in str(err.value)
        assert t.cluster_deadlines().tolist() == term
        _same(t.tick(snap, resident_workers=True), want)
        # a sharded context
        sh.cluster_upload(snap)
        sh._lib.hqtick_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        assert sh._lib.hqtick_set_shard(sh._ctx, 0, 2) == 0
        with pytest.raises(HqTickError) as err:
            sh.cluster_set_clock(now)
        assert err.value.code == abi.HQTICK_E_UNSUPPORTED
        with pytest.raises(HqTickError):
            sh.cluster_deadlines()  # still outside clock mode
        # a placement waits for its consume (two-call form, assignment ledger on)
        led.cluster_upload(snap); led.upload_ready(*tasks); led.assigned_enable([]); led.cluster_set_clock(now)
        sc = snap.to_c(resident_workers=True)
        sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
        led.tick_raw(sc, resident=True)
        with pytest.raises(HqTickError) as err:
            led.cluster_set_clock(now + 100 * S)
        assert err.value.code == abi.HQTICK_E_INVALID and "pending" in str(err.value)
        led.ready_consume_last()
        led.cluster_set_clock(now + 100 * S)
        assert led.cluster_deadlines().tolist() == term
        # hqtick_cluster_upload leaves clock mode
        t.cluster_upload(snap)
        with pytest.raises(HqTickError):
            t.cluster_deadlines()
        _same(t.tick(snap), want)
    finally:
        for x in (plain, t, sh, led):
            x.close()


def test_no_clock_no_change():
    """a context that never sets the clock launches no k_clock_rows and times the same kernels as before; one that does launches it only when the clock, a deadline,
    the membership or the request table changed since its last run"""
    now = 0
    ids, term = list(range(1, 9)), [now + (20 * k + 5) * S for k in range(8)]
    total = np.tile(np.asarray([8, 1, 32], np.uint64) * np.uint64(workloads.FR), (8, 1))
    tasks = _tasks(5_000, [0, 1, 2, 3, 4], seed=8)
    snap = _snap(ids, total, term, now, REQ3, tasks)
    off, on = _tick(measure=True), _tick(measure=True)
    launches = lambda t: (setattr(t._lib.hqtick_debug_clock_launches, "argtypes", [C.c_void_p]), t._lib.hqtick_debug_clock_launches(t._ctx))[1]
    timed = lambda t: sorted(k for k in ("distinct_us", "level_hist_us", "scan_us", "block_solve_us", "select_us", "sweep_us", "other_us") if t.kernel_stats()[k] > 0)  # the kernels the timing switch brackets
    try:
        off.cluster_upload(snap); on.cluster_upload(snap)
        on.cluster_set_clock(now)
        for k in range(3):
            a, b = off.tick(snap, resident_workers=True), on.tick(snap, resident_workers=True)
            _same(a, b)
            assert timed(off) == timed(on)
            assert launches(off) == 0 and launches(on) == 1  # the second and third tick found nothing changed
        on.cluster_set_clock(now)  # the same time again
        on.tick(snap, resident_workers=True)
        assert launches(on) == 1
        on.cluster_set_clock(now + 1)
        on.tick(snap, resident_workers=True)
        assert launches(on) == 2
        on.cluster_update_workers([2], total[2:3], remaining_ns=[9 * S])  # a deadline
        on.tick(snap, resident_workers=True)
        assert launches(on) == 3
        more = dataclasses.replace(snap, _keep=[], requests=REQ3 + [[_variant([(0, 1)], 50)]])  # the request table
        on.tick(more, resident_workers=True)
        assert launches(on) == 4
        on.cluster_remove_workers([ids[-1]])  # the membership
        on.tick(_snap(ids[:-1], total[:-1], term[:-1], now, more.requests, tasks), resident_workers=True)
        assert launches(on) == 5
        off.cluster_update_workers([2], total[2:3], remaining_ns=[9 * S])  # outside clock mode the same call writes the column itself
        off.tick(snap, resident_workers=True)
        assert launches(off) == 0
    finally:
        off.close(); on.close()
