"""hqtick_query_resident (ABI 11): the autoalloc query (compute_new_worker_query, scheduler/query.rs) answered from the resident ready set in HBM.
Checked three ways: the reference's query vectors through a backend that holds its ready set only on the device; an exact A/B against hqtick_query
on the equivalent full snapshot at every kind of resident state (upload, tombstones, consume-in-tick, removes, appended adds, the dependency graph,
the full c3p set); and ticks of a context that is queried before every tick equal to those of a context that is not."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import golden_cases
from hyperqueue_amd import abi, workloads
from hyperqueue_amd.tick import HqTickError, Tick

pytestmark = pytest.mark.gpu

UNIT = abi.HQ_FRACTIONS_PER_UNIT
QUERY_CASES = [c for c in golden_cases.ALL_CASES if c.__name__.startswith("test_query_")]


def with_ready(snap: abi.Snapshot, ids, prio, rq) -> abi.Snapshot:
    return dataclasses.replace(snap, task_id=np.asarray(ids, np.uint64), task_priority=np.asarray(prio, np.uint64), task_rq=np.asarray(rq, np.uint32), _keep=[])


def stripped(snap: abi.Snapshot) -> abi.Snapshot:
    """the snapshot a resident host sends: no task columns"""
    return with_ready(snap, np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


def without_workers(snap: abi.Snapshot) -> abi.Snapshot:
    R = snap.n_resources
    return dataclasses.replace(snap, worker_id=np.zeros(0, np.uint32), worker_total=np.zeros((0, R), np.uint64), worker_free=np.zeros((0, R), np.uint64),
                               worker_remaining_ns=np.zeros(0, np.int64), worker_min_utilization=np.zeros(0, np.float32), worker_flags=np.zeros(0, np.uint8),
                               worker_group=np.zeros(0, np.uint32), blocked=[], assigned=[], prefilled=[], prefill={}, worker_map_rank=None, retracting=[], _keep=[])


def bincount(snap: abi.Snapshot) -> np.ndarray:
    return np.bincount(np.asarray(snap.task_rq, np.int64), minlength=len(snap.requests)).astype(np.uint64)


# ---------------------------------------------------------------------------------------------- 1. the reference's query vectors
class ResidentQueryBackend:
    """ticks through hqtick_run; queries by uploading the snapshot's ready set and asking hqtick_query_resident with the task columns stripped"""

    def __init__(self):
        self.t = Tick(abi.make_config())
        self.q = Tick(abi.make_config())

    def tick(self, snap):
        return self.t.tick(snap)

    def query(self, snap, ids, totals, rem, mu):
        self.q.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        loaded, opt, rq_ready = self.q.query_resident(stripped(snap), ids, totals, rem, mu)
        assert (rq_ready == bincount(snap)).all(), (rq_ready, bincount(snap))
        return loaded, opt


@pytest.fixture(scope="module")
def qbackend():
    return ResidentQueryBackend()


@pytest.mark.parametrize("case", QUERY_CASES, ids=lambda f: f.__name__)
def test_reference_query_vectors(case, qbackend):
    case(qbackend)


def test_all_reference_query_cases_are_run():
    assert len(QUERY_CASES) == 22


# ---------------------------------------------------------------------------------------------- 2. A/B against hqtick_query
def query_shapes(R: int):
    """(ids, totals [n, R], remaining, min_util) per shape: plain, partial, time limit, min_utilization, mixed"""
    def rows(n, cpus, rest=0):
        t = np.full((n, R), rest, np.uint64)
        t[:, 0] = cpus * UNIT
        return t
    base = 1 << 20  # fake ids above every real worker id
    ids = np.arange(base, base + 6, dtype=np.uint32)
    no_limit = np.full(6, abi.HQ_NO_TIME_LIMIT, np.int64)
    zero_mu = np.zeros(6, np.float32)
    return {
        "plain": (ids, rows(6, 16), no_limit, zero_mu),
        "partial": (ids, rows(6, 8, abi.HQ_AMOUNT_MAX), no_limit, zero_mu),
        "time_limit": (ids, rows(6, 64, 512 * UNIT), np.full(6, 100 * 10**9, np.int64), zero_mu),
        "min_util": (ids, rows(6, 32, abi.HQ_AMOUNT_MAX), no_limit, np.full(6, 0.5, np.float32)),
        "mixed": (ids, np.concatenate([rows(3, 4, abi.HQ_AMOUNT_MAX), rows(3, 128, 8 * UNIT)]), np.asarray([abi.HQ_NO_TIME_LIMIT] * 3 + [3600 * 10**9] * 3, np.int64),
                  np.asarray([0, 0.9, 0, 0, 0.25, 1.0], np.float32)),
    }


def assert_ab(t: Tick, full: abi.Snapshot, ref: Tick, shapes=None, what=""):
    """query_resident on t's resident set == hqtick_query on `full` (the same ready set as columns), for every query shape"""
    want_rq = bincount(full)
    for name, (ids, tot, rem, mu) in (shapes or query_shapes(full.n_resources)).items():
        got_l, got_o, rq_ready = t.query_resident(stripped(full), ids, tot, rem, mu)
        want_l, want_o = ref.query(full, ids, tot, rem, mu)
        assert got_l.tobytes() == want_l.tobytes() and got_o == want_o, (what, name, got_l, want_l, got_o, want_o)
        assert (rq_ready == want_rq).all(), (what, name, rq_ready, want_rq)


class Live:
    """host-side record of the resident set (id -> (priority, rq)) to build the equivalent full snapshot from"""

    def __init__(self, snap):
        self.m = {int(i): (int(p), int(q)) for i, p, q in zip(snap.task_id, snap.task_priority, snap.task_rq)}

    def take(self, res: abi.Result):
        for recs in res.records:
            for (tid, _, _) in recs:
                del self.m[tid]
        for (tid, _) in res.mn:
            del self.m[tid]

    def add(self, ids, prio, rq):
        for i, p, q in zip(ids, prio, rq):
            self.m[int(i)] = (int(p), int(q))

    def remove(self, ids):
        for i in ids:
            del self.m[int(i)]

    def full(self, snap):
        ids = sorted(self.m)
        return with_ready(snap, ids, [self.m[i][0] for i in ids], [self.m[i][1] for i in ids])


@pytest.fixture(scope="module")
def ref():
    t = Tick(abi.make_config(time_limit_s=20.0))
    yield t
    t.close()


def test_ab_through_resident_deltas(ref):
    """upload; ticks + consume with tombstones left in the columns; a remove; an appended packed add — A/B at each"""
    cfg = abi.make_config(time_limit_s=20.0)
    snap = workloads.make("c3p", n_tasks=20_000, n_workers=16, seed=3)
    t = Tick(cfg)
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    live = Live(snap)
    assert_ab(t, live.full(snap), ref, what="upload")
    empty = stripped(snap)
    for step in range(3):
        r = t.tick(empty, resident=True)
        t.ready_consume_last()
        live.take(r)
        assert t.ready_count() == len(live.m)
        assert_ab(t, live.full(snap), ref, what=f"tick {step}")
    victims = np.asarray(sorted(live.m)[::97][:60], np.uint64)
    assert t.ready_remove(victims) == len(victims)
    live.remove(victims)
    assert_ab(t, live.full(snap), ref, what="remove")
    low = np.arange(1, 201, dtype=np.uint64)   # ids below every resident one (job 0): merged into new columns, which leaves room behind them
    assert not np.isin(low, snap.task_id).any()
    t.ready_add(low, np.full(200, int(snap.task_priority[0]), np.uint64), np.arange(200, dtype=np.uint32) % len(snap.requests))
    live.add(low, [int(snap.task_priority[0])] * 200, np.arange(200) % len(snap.requests))
    assert_ab(t, live.full(snap), ref, what="merge")
    next_id = int(snap.task_id.max()) + 1
    rng = np.random.default_rng(7)
    n = 500
    rq16 = rng.integers(0, len(snap.requests), n).astype(np.uint16)
    p0 = int(snap.task_priority.max()) + 1   # a new top level
    apps = t.kernel_stats()["ready_appends"]
    t.ready_add_packed([(next_id, n)], [(p0, n)], rq16)
    assert t.kernel_stats()["ready_appends"] == apps + 1   # appended behind the columns, not merged
    live.add(range(next_id, next_id + n), [p0] * n, rq16)
    assert_ab(t, live.full(snap), ref, what="append")
    r = t.tick(empty, resident=True)   # and the set still ticks
    t.ready_consume_last()
    live.take(r)
    assert_ab(t, live.full(snap), ref, what="after append tick")
    t.close()


def test_ab_under_consume_in_tick(ref):
    cfg = abi.make_config(time_limit_s=20.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK)
    snap = workloads.make("c3", n_tasks=30_000, n_workers=24, seed=5)
    t = Tick(cfg)
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    live = Live(snap)
    for step in range(3):
        r = t.tick(stripped(snap), resident=True)   # no consume: the tick took its tasks itself, nothing is pending
        live.take(r)
        assert_ab(t, live.full(snap), ref, what=f"consume-in-tick {step}")
    t.close()


def test_ab_multi_node_requests(ref):
    """the query shapes of the reference's multi-node case on a resident set with multi-node queues (their workers are busy: query.rs answers)"""
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB

    env = SchedEnv()
    env.new_workers_cpus([4, 4, 4])
    env.new_tasks(5, TB().n_nodes(3)); env.new_tasks(10, TB().n_nodes(6)); env.new_tasks(20, TB().n_nodes(3).user_priority(10))
    env.new_tasks(30, TB().cpus(2)); env.new_tasks(7, TB().cpus(1).user_priority(3))
    env.schedule(ref)
    snap = env.snapshot()
    t = Tick(abi.make_config())
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    R = snap.n_resources
    ids = np.arange(1000, 1004, dtype=np.uint32)
    tot = np.zeros((4, R), np.uint64); tot[:, 0] = 4 * UNIT
    shapes = {"mn_plain": (ids, tot, np.full(4, abi.HQ_NO_TIME_LIMIT, np.int64), np.zeros(4, np.float32)),
              "mn_time": (ids, tot, np.full(4, 50 * 10**9, np.int64), np.full(4, 0.5, np.float32))}
    assert_ab(t, snap, ref, shapes, what="multi-node")
    t.close()


def test_ab_inside_the_graph_loop(ref):
    """config-5 shape: tasks enter the resident set through hqtick_graph_add_tasks / hqtick_graph_finish; A/B after every finish"""
    from oracle.graph_oracle import GraphOracle

    n, W = 3_000, 4
    ids, prio, rq, off, dep = workloads.make_dag(n, seed=3)
    rq = (rq % np.uint32(3)).astype(np.uint32)
    meta = {int(i): (int(p), int(q)) for i, p, q in zip(ids, prio, rq)}
    g = GraphOracle()
    g.on_new_tasks([(int(ids[i]), int(prio[i]), int(rq[i]), [int(x) for x in dep[off[i]:off[i + 1]]]) for i in range(n)])
    T = Tick(abi.make_config(time_limit_s=20.0))
    T.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    T.graph_add_tasks(ids, prio, rq, (off, dep))
    drv = workloads.DagChurn(n_workers=W, churn=0.25, seed=1)
    steps, checked = 0, 0
    while g.tasks and steps < 12:
        got = T.tick(drv.snapshot(), resident=True)
        T.ready_consume_last()
        rec_off = np.zeros(W + 1, np.int64)
        rec_off[1:] = np.cumsum([len(r) for r in got.records])
        rec_task = np.asarray([t for r in got.records for (t, _, _) in r], np.uint64)
        g.take_from_ready(rec_task.tolist())
        finished, returned = drv.after_tick(rec_off, rec_task)
        for i in returned.tolist():
            g.ready[i] = meta[i]
        if len(returned):
            T.ready_add(returned, [meta[int(i)][0] for i in returned], [meta[int(i)][1] for i in returned])
        g.task_finished(finished.tolist())
        if len(finished):
            T.graph_finish(finished)
        rid = sorted(g.ready)
        if rid:
            full = drv.snapshot(rid, [g.ready[i][0] for i in rid], [g.ready[i][1] for i in rid])
            assert_ab(T, full, ref, what=f"graph step {steps}")
            checked += 1
        steps += 1
    assert checked >= 3
    T.close()


def test_ab_full_c3p(ref):
    """the full c3p ready set: 1 M tasks, three priority levels"""
    snap = workloads.make("c3p")
    assert len(snap.task_id) == 1_000_000 and len(np.unique(snap.task_priority)) == 3
    t = Tick(abi.make_config(time_limit_s=20.0))
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    assert_ab(t, snap, ref, what="c3p")
    t.close()


# ---------------------------------------------------------------------------------------------- 3. no interference with the ticks
def assert_same_tick(got, want, step):
    assert got.status == want.status and got.is_optimal == want.is_optimal and got.counts == want.counts, step
    assert got.records == want.records and got.retracts == want.retracts and sorted(got.redirects) == sorted(want.redirects), step


def test_queries_leave_the_ticks_alone():
    cfg = abi.make_config(time_limit_s=20.0)
    snap = workloads.make("c3p", n_tasks=40_000, n_workers=24, seed=11)
    a, b = Tick(cfg), Tick(cfg)
    for t in (a, b):
        t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    empty = stripped(snap)
    ids, tot, rem, mu = query_shapes(snap.n_resources)["mixed"]
    rng = np.random.default_rng(3)
    next_id = int(snap.task_id.max()) + 1
    for step in range(12):
        b.query_resident(empty, ids, tot, rem, mu)
        ra = a.tick(empty, resident=True)
        rb = b.tick(empty, resident=True)
        assert_same_tick(rb, ra, step)
        if step % 4 == 1:   # a query between the tick and its consume: refused, and the consume after it still replays the tick's selection
            with pytest.raises(HqTickError) as e:
                b.query_resident(empty, ids, tot, rem, mu)
            assert e.value.code == abi.HQTICK_E_INVALID and "consume" in str(e.value)
        a.ready_consume_last(); b.ready_consume_last()
        assert a.ready_count() == b.ready_count(), step
        if step % 3 == 2:
            n = int(rng.integers(1, 300))
            rq16 = rng.integers(0, len(snap.requests), n).astype(np.uint16)
            for t in (a, b):
                t.ready_add_packed([(next_id, n)], [(int(snap.task_priority[0]), n)], rq16)
            next_id += n
    a.close(); b.close()


def test_query_without_a_resident_set_is_refused():
    snap = workloads.make("c3", n_tasks=100, n_workers=4)
    t = Tick(abi.make_config())
    ids, tot, rem, mu = query_shapes(snap.n_resources)["plain"]
    with pytest.raises(HqTickError) as e:
        t.query_resident(stripped(snap), ids, tot, rem, mu)
    assert e.value.code == abi.HQTICK_E_INVALID
    t.tick(snap)   # a snapshot tick leaves no resident set either
    with pytest.raises(HqTickError) as e:
        t.query_resident(stripped(snap), ids, tot, rem, mu)
    assert e.value.code == abi.HQTICK_E_INVALID
    t.close()


# ---------------------------------------------------------------------------------------------- 4. real workers are not read
def test_real_workers_do_not_change_the_answer(ref):
    snap = workloads.make("c3p", n_tasks=50_000, n_workers=32, seed=2)
    t = Tick(abi.make_config(time_limit_s=20.0))
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    t.cluster_upload(snap)
    for name, (ids, tot, rem, mu) in query_shapes(snap.n_resources).items():
        listed = t.query_resident(stripped(snap), ids, tot, rem, mu)
        none = t.query_resident(stripped(without_workers(snap)), ids, tot, rem, mu)
        resident = t.query_resident(stripped(snap), ids, tot, rem, mu, resident_workers=True)
        for other in (none, resident):
            assert listed[0].tobytes() == other[0].tobytes() and listed[1] == other[1] and (listed[2] == other[2]).all(), name
    t.close()


def test_a_shard_replica_answers_as_a_single_context(ref):
    snap = workloads.make("c3p", n_tasks=20_000, n_workers=16, seed=4)
    t = Tick(abi.make_config(time_limit_s=20.0))
    t._lib.hqtick_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    assert t._lib.hqtick_set_shard(t._ctx, 1, 2) == 0
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    assert_ab(t, snap, ref, what="shard 1 of 2")
    t.close()


def test_config_written_for_abi_10_is_accepted():
    cfg = abi.make_config()
    cfg.abi_version = 10
    t = Tick(cfg)
    t.close()
