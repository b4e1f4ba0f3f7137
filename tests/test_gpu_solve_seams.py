"""Seams of the placement's device side (hqsolve::Solver: the block solvers, the exchange, the replica predicate) that the scenario tests cross without pinning
them: k_block_solve with and without its profile, a step budget of 1, queries between ticks (both forms create the sub-context), the replica predicate as a
callback or a communicator switches it on and off, and an exchange that fails.  Small on purpose: 48 workers of the reduced c3 family, a few thousand tasks."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads

pytestmark = pytest.mark.gpu

UNIT = abi.HQ_FRACTIONS_PER_UNIT
W, N = 48, 4000


def _cfg(flags=0):
    return abi.make_config(time_limit_s=20.0, flags=flags)


def _oracle():
    from oracle.oracle import Oracle

    return Oracle(_cfg(), canonical=True)


def _same(got, want):
    assert got.status == want.status and got.is_optimal == want.is_optimal and got.batches == want.batches and got.counts == want.counts
    assert got.records == want.records and got.retracts == want.retracts and (got.new_free == want.new_free).all()


def _empty(snap):
    return dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))


def _without(snap, res):
    """the snapshot with the tasks `res` handed out gone from its ready set (the workers as they were)"""
    taken = np.asarray(sorted(t for recs in res.records for (t, _v, _k) in recs), np.uint64)
    keep = ~np.isin(snap.task_id, taken)
    return dataclasses.replace(snap, _keep=[], task_id=snap.task_id[keep], task_priority=snap.task_priority[keep], task_rq=snap.task_rq[keep]), len(taken)


def _set_shard(t, index, count):
    t._lib.hqtick_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    assert t._lib.hqtick_set_shard(t._ctx, index, count) == 0


def _comm_init(t):
    """a communicator of one rank (what one GPU can run)"""
    uid = (C.c_ubyte * 128)()
    t._lib.hqtick_comm_unique_id.argtypes = [C.c_void_p]
    t._lib.hqtick_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    assert t._lib.hqtick_comm_unique_id(uid) == 0
    assert t._lib.hqtick_comm_init(t._ctx, uid, 0, 1) == 0


def _comm_destroy(t):
    t._lib.hqtick_comm_destroy.argtypes = [C.c_void_p]
    assert t._lib.hqtick_comm_destroy(t._ctx) == 0


@pytest.fixture(scope="module")
def steady():
    """a separable tick: 48 busy workers, about one class each — and the canonical oracle's answer to it"""
    snap = workloads.make_steady("c3", seed=0, n_tasks=N, n_workers=W)
    return snap, _oracle().tick(snap)


# ---------------------------------------------------------------------------------------------- 1. device blocks, with and without the profile
@pytest.mark.parametrize("profile", [False, True], ids=["plain", "profile"])
def test_device_blocks(profile, steady, monkeypatch):
    from hyperqueue_amd.tick import Tick

    snap, want = steady
    monkeypatch.setenv("HQTICK_BLOCK_MIN_CLASSES", "1")  # (read when the context is created)
    if profile:
        monkeypatch.setenv("HQTICK_BLOCK_PROFILE", "1")
    t = Tick(_cfg(), measure=profile)  # hqtick_block_profile_last is a measurement hook: the same objects plus include/hqtick_debug.h
    got = t.tick(snap)
    ks = t.kernel_stats()
    print(f"device blocks{', profile' if profile else ''}: {ks['n_classes_device']} classes on the device, {ks['n_classes_host']} on the host, block_solve_us > 0: {ks['block_solve_us'] > 0}")
    _same(got, want)
    assert got.is_canonical
    assert ks["n_classes_device"] > 0 and ks["block_solve_us"] > 0
    if profile:
        n = C.c_uint32(0)
        t._lib.hqtick_block_profile_last.restype = C.POINTER(C.c_uint64)
        t._lib.hqtick_block_profile_last.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        p = t._lib.hqtick_block_profile_last(t._ctx, C.byref(n))
        print(f"profile: {n.value} classes, pointer set: {bool(p)}")
        assert bool(p) and n.value == ks["n_classes_device"]
    t.close()


# ---------------------------------------------------------------------------------------------- 2. a budget of one step
def test_tiny_budget_hands_every_class_to_the_host(steady, monkeypatch):
    from hyperqueue_amd.tick import Tick

    snap, want = steady
    monkeypatch.setenv("HQTICK_BLOCK_MIN_CLASSES", "1")
    monkeypatch.setenv("HQTICK_BLOCK_BUDGET", "1")
    t = Tick(_cfg())
    got = t.tick(snap)
    ks = t.kernel_stats()
    print(f"budget 1: {ks['n_classes_device']} classes on the device, {ks['n_classes_host']} on the host")
    assert ks["n_classes_host"] > 0
    _same(got, want)  # the placement of case 1
    t.close()


# ---------------------------------------------------------------------------------------------- 3. queries between ticks
def test_queries_between_ticks_leave_no_trace(steady, monkeypatch):
    """a tick, hqtick_query (its first call creates the sub-context), hqtick_query_resident, the next tick: the ticks equal those of a context nobody queried, and
    both query forms load the same fake workers"""
    from hyperqueue_amd.tick import Tick

    snap, want = steady
    monkeypatch.setenv("HQTICK_BLOCK_MIN_CLASSES", "1")
    R = snap.n_resources
    ids = np.arange(4, dtype=np.uint32) + (1 << 20)
    totals = np.zeros((4, R), np.uint64)
    totals[0] = snap.worker_total[0]; totals[1, 0] = 1 * UNIT; totals[2, 0] = 16 * UNIT; totals[2, 2] = 8 * UNIT  # a whole worker, one cpu, cpus + mem, nothing
    cfg = _cfg(abi.HQTICK_FLAG_CONSUME_IN_TICK)
    results = {}
    for queried in (True, False):
        t = Tick(cfg)
        t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        r1 = t.tick(_empty(snap), resident=True)
        left, n_taken = _without(snap, r1)
        if queried:
            a, a_opt = t.query(left, ids, totals)
            b, b_opt, rq_ready = t.query_resident(_empty(snap), ids, totals)
            print(f"queries: hqtick_query loads {a.astype(int).tolist()}, hqtick_query_resident loads {b.astype(int).tolist()}, optimal {a_opt} {b_opt}, {int(rq_ready.sum())} ready")
            assert a.tolist() == b.tolist() and a_opt == b_opt and a.any() and not a.all()
            assert int(rq_ready.sum()) == N - n_taken == t.ready_count()
        r2 = t.tick(_empty(snap), resident=True)
        results[queried] = (r1, r2)
        t.close()
    _same(results[True][0], want)
    _same(results[True][0], results[False][0]); _same(results[True][1], results[False][1])
    n_next = sum(len(r) for r in results[True][1].records)
    print(f"queries: first tick hands out {sum(len(r) for r in results[True][0].records)}, the next {n_next}")
    assert n_next > 0


# ---------------------------------------------------------------------------------------------- 4. the replica predicate, as it switches
@pytest.mark.parametrize("how", ["callback", "communicator"])
def test_replica_predicate_refuses_the_ledger_and_lets_it_back(how):
    from hyperqueue_amd.tick import HqTickError, Tick

    snap = workloads.make("c3", seed=2, n_tasks=N, n_workers=W)  # idle workers: the ledger starts empty
    single = Tick(_cfg())
    want = single.tick(snap)  # (4000 tasks do not saturate 48 idle workers: the placement is optimal, not canonical, so the reference is the library's own single scheduler)
    single.close()

    def ledger_tick(t):
        sc = snap.to_c(resident_workers=True)
        sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
        return abi.parse_result(t.tick_raw(sc), W, snap.n_resources)

    t = Tick(_cfg())
    t.cluster_upload(snap)
    t.assigned_enable([])
    if how == "callback":
        t.set_exchange(lambda s, r, n: 0)
    else:
        _comm_init(t)
    with pytest.raises(HqTickError) as ei:
        ledger_tick(t)
    print(f"ledger, {how} set: {ei.value}")
    assert ei.value.code == abi.HQTICK_E_UNSUPPORTED and str(ei.value) == f"hqtick error {abi.HQTICK_E_UNSUPPORTED}: assignment ledger on a sharded or replica context"
    if how == "callback":
        t.set_exchange(None)
    else:
        _comm_destroy(t)
    got = ledger_tick(t)  # a single scheduler again
    print(f"ledger, {how} gone: {sum(len(r) for r in got.records)} records, {t.assigned_count()} in the ledger")
    _same(got, want)
    assert t.assigned_count() == sum(1 for recs in got.records for (_t, _v, k) in recs if k == abi.HQ_REC_ASSIGN) > 0
    t.close()


@pytest.mark.parametrize("how", ["callback", "communicator"])
def test_replica_predicate_overrides_certificate_only(how):
    """HQTICK_FLAG_CERTIFICATE_ONLY is one scheduler's: a replica returns the canonical point.  The small coupled tick of tests/test_gpu_price.py, where the flag shows."""
    from hyperqueue_amd.tick import Tick

    ids, prio, rq, _off, _dep = workloads.make_dag(200_000, seed=0)
    snap = workloads.DagChurn(n_workers=1024, churn=0.1, seed=0).snapshot(ids[:89], prio[:89], (rq[:89] % 8).astype(np.uint32))
    plain, flagged = Tick(abi.make_config(time_limit_s=5.0)), Tick(abi.make_config(time_limit_s=5.0, flags=abi.HQTICK_FLAG_CERTIFICATE_ONLY))
    exact, quick = plain.tick(snap), flagged.tick(snap)
    plain.close(); flagged.close()
    assert exact.is_canonical and not quick.is_canonical  # (the flag shows on this tick)
    t = Tick(abi.make_config(time_limit_s=5.0, flags=abi.HQTICK_FLAG_CERTIFICATE_ONLY))
    if how == "callback":
        t.set_exchange(lambda s, r, n: 0)
    else:
        _comm_init(t)
    as_replica = t.tick(snap)
    if how == "callback":
        t.set_exchange(None)
    else:
        _comm_destroy(t)
    alone = t.tick(snap)
    t.close()
    print(f"certificate only, {how}: canonical {as_replica.is_canonical} while set, {alone.is_canonical} once gone")
    assert as_replica.is_canonical == exact.is_canonical and as_replica.counts == exact.counts and as_replica.records == exact.records
    assert alone.is_canonical == quick.is_canonical and alone.counts == quick.counts


# ---------------------------------------------------------------------------------------------- 5. an exchange that fails
def _failing(calls):
    def fn(_send, _recv, _n):
        calls.append(1)
        return 1  # at once: nothing waits
    return fn


def test_failed_exchange_plain_tick(steady, monkeypatch):
    """rank 0 of 2 whose exchange fails in the class blocks' all-gather.  What the library makes of it was recorded from the parent commit's run: no error — a launch
    whose exchange fails counts as a failed launch, the host solves every class, and the tick returns this rank's records of the canonical placement."""
    from hyperqueue_amd.tick import Tick

    snap, want = steady
    monkeypatch.setenv("HQTICK_BLOCK_MIN_CLASSES", "1")
    monkeypatch.setenv("HQTICK_SHARD_MIN_CLASSES", "1")
    t = Tick(_cfg())
    calls = []
    _set_shard(t, 0, 2)
    t.set_exchange(_failing(calls))
    got = t.tick(snap)
    ks = t.kernel_stats()
    print(f"failed exchange: status {got.status}, callback called {len(calls)} time(s), {ks['n_classes_device']} classes on the device, {ks['n_classes_host']} on the host, "
          f"{ks['exchange_calls']} exchanges counted")
    assert len(calls) == 1 and ks["exchange_calls"] == 0 and ks["n_classes_device"] == 0 and ks["n_classes_host"] > 0
    assert got.status == want.status and got.is_optimal and got.is_canonical and got.batches == want.batches and got.counts == want.counts
    from hyperqueue_amd.hbmap import hash_u32

    mine = [recs if hash_u32(int(wid)) % 2 == 0 else [] for wid, recs in zip(snap.worker_id, want.records)]  # hqtick_set_shard: a worker is rank FxHash(id) % world's
    assert got.records == mine
    t.set_exchange(None); _set_shard(t, 0, 1)
    _same(t.tick(snap), want)
    t.close()


def test_failed_exchange_consume_in_tick(steady, monkeypatch):
    """the same with HQTICK_FLAG_CONSUME_IN_TICK on a resident ready set.  Recorded from the parent commit's run: status 0 here as well (868 records of this rank, 1985 of
    the 4000 tasks left) — a failed exchange in the class blocks is no error, so the tick keeps what it took and the put-back of a failed tick ("... is back in the
    resident ready set") is not reached this way.  What is pinned is that outcome: this rank's records of the canonical placement, the whole placement's tasks gone
    from the ready set, and the next tick, as a single scheduler again, equal to that of a context that never had an exchange."""
    from hyperqueue_amd.hbmap import hash_u32
    from hyperqueue_amd.tick import HqTickError, Tick

    snap, want = steady
    n_want = sum(len(r) for r in want.records)
    ref = Tick(_cfg(abi.HQTICK_FLAG_CONSUME_IN_TICK))  # the same two ticks of one scheduler without an exchange
    ref.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    _same(ref.tick(_empty(snap), resident=True), want)
    want_next = ref.tick(_empty(snap), resident=True)
    ref.close()
    monkeypatch.setenv("HQTICK_BLOCK_MIN_CLASSES", "1")
    monkeypatch.setenv("HQTICK_SHARD_MIN_CLASSES", "1")
    t = Tick(_cfg(abi.HQTICK_FLAG_CONSUME_IN_TICK))
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    calls = []
    _set_shard(t, 0, 2)
    t.set_exchange(_failing(calls))
    try:
        got = t.tick(_empty(snap), resident=True)
        outcome = f"status {got.status}, {sum(len(r) for r in got.records)} records"
    except HqTickError as e:
        got, outcome = None, str(e)
    print(f"failed exchange, consume-in-tick: {outcome}; callback called {len(calls)} time(s), {t.ready_count()} left")
    assert got is not None and len(calls) == 1
    assert got.status == want.status and got.is_optimal and got.is_canonical and got.counts == want.counts
    assert got.records == [recs if hash_u32(int(wid)) % 2 == 0 else [] for wid, recs in zip(snap.worker_id, want.records)]
    assert t.ready_count() == N - n_want
    t.set_exchange(None); _set_shard(t, 0, 1)
    _same(t.tick(_empty(snap), resident=True), want_next)
    t.close()
