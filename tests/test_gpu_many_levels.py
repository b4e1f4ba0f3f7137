"""Ready sets beyond the dense scan's caps (more than 4096 distinct priorities, or more than 16384 (level, request) groups) take the ordered view of
the ready set instead of failing with HQTICK_E_CAPACITY.  Each such tick must equal the canonical oracle; on small inputs the view,
forced by HQTICK_ORDERED_VIEW=1, must give byte-identical results to the dense path."""
import ctypes as C

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads
from hyperqueue_amd.core import priority_from_user

pytestmark = pytest.mark.gpu


def assert_same(got: abi.Result, want: abi.Result):
    assert got.status == want.status
    assert got.batches == want.batches
    assert got.counts == want.counts
    assert got.records == want.records
    assert got.retracts == want.retracts
    assert sorted(got.redirects) == sorted(want.redirects)
    assert got.mn == want.mn
    assert (got.new_free == want.new_free).all()


def many_levels(n_levels: int, n_classes: int, n_tasks: int, n_workers: int, seed: int = 0, cpu_div: int = 16, one_cpu: bool = False) -> abi.Snapshot:
    """c3's cluster at reduced size (8 cpus per worker, so that the canonical oracle stays quick) and a ready set in which every one of n_levels user
    priorities occurs, spread over n_classes request classes"""
    snap = workloads.make("c3", seed=seed, n_tasks=n_tasks, n_workers=n_workers)
    rng = np.random.default_rng(n_levels * 7 + n_classes + seed)
    n = len(snap.task_id)
    if n_classes != 8:
        snap.requests = [[workloads._variant([(0, 1 if one_cpu else 1 + (q % 4))])] for q in range(n_classes)]
    snap.task_rq = rng.integers(0, n_classes, n).astype(np.uint32)
    lv = np.concatenate([np.arange(n_levels), rng.integers(0, n_levels, n - n_levels)]) if n > n_levels else np.arange(n)
    rng.shuffle(lv)
    snap.task_priority = np.asarray([priority_from_user(int(p)) for p in lv], np.uint64)
    snap.worker_total = snap.worker_total.copy()
    snap.worker_total[:, 0] //= cpu_div
    snap.worker_free = snap.worker_total.copy()
    return snap


def last_order(t):
    f = t._lib.hqtick_debug_last_order
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    runs, levels, us = C.c_uint32(), C.c_uint32(), C.c_double()
    on = f(t._ctx, C.byref(runs), C.byref(levels), C.byref(us))
    return on, runs.value, levels.value, us.value


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import Oracle

    return Oracle(abi.make_config(time_limit_s=60.0), canonical=True)


SHAPES = [(4097, 1, 4200, 8), (6000, 2, 6000, 8), (20_000, 1, 20_000, 8)]


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("n_levels,n_classes,n_tasks,n_workers", SHAPES)
def test_a_tick_beyond_the_dense_caps_equals_the_oracle(n_levels, n_classes, n_tasks, n_workers, resident, oracle):
    from hyperqueue_amd.tick import Tick

    snap = many_levels(n_levels, n_classes, n_tasks, n_workers)
    want = oracle.tick(snap)
    t = Tick(abi.make_config(time_limit_s=60.0), measure=True)
    try:
        if resident:
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
        got = t.tick(snap, resident=resident)
        on, runs, levels, _us = last_order(t)
        assert on == 1 and levels == len(np.unique(snap.task_priority))
        assert runs == len(set(zip(snap.task_rq.tolist(), snap.task_priority.tolist())))
        assert_same(got, want)
        again = t.tick(snap, resident=resident)   # (the next tick goes straight to the view)
        assert_same(again, want)
    finally:
        t.close()


def test_retracting_tasks_on_the_view(oracle):
    """Retracting tasks: their queue position comes from the view's inverse permutation"""
    from hyperqueue_amd.tick import Tick

    snap = many_levels(4097, 1, 4200, 8, seed=3)
    order = np.lexsort((snap.task_id, ~snap.task_priority))   # the queue's take order: priority descending, then id
    pick = np.sort(snap.task_id[order[[0, 5, 17, 300, 4000]]])
    snap.retracting = [(int(tid), i % len(snap.worker_id), abi.HQ_NO_WORKER, 0) for i, tid in enumerate(pick.tolist())]
    want = oracle.tick(snap)
    t = Tick(abi.make_config(time_limit_s=60.0), measure=True)
    try:
        got = t.tick(snap)
        assert last_order(t)[0] == 1
        assert_same(got, want)
    finally:
        t.close()


@pytest.mark.parametrize("n_levels,n_classes", [(1, 8), (3, 8), (4, 8), (5, 8), (9, 3), (3, 20), (70, 8)])
def test_the_view_equals_the_dense_scan_on_the_discovery_grid(n_levels, n_classes, monkeypatch):
    from hyperqueue_amd.tick import Tick

    snap = workloads.make("c3", seed=5, n_tasks=6_000, n_workers=6)
    rng = np.random.default_rng(n_levels * 100 + n_classes)
    if n_classes != 8:
        snap.requests = [[workloads._variant([(0, 1 + (q % 4))])] for q in range(n_classes)]
    snap.task_rq = rng.integers(0, n_classes, len(snap.task_id)).astype(np.uint32)
    snap.task_priority = np.asarray([priority_from_user(int(p)) for p in rng.integers(0, n_levels, len(snap.task_id))], np.uint64)
    outs = []
    for view in (False, True):
        monkeypatch.setenv("HQTICK_ORDERED_VIEW", "1" if view else "0")
        t = Tick(abi.make_config(time_limit_s=20.0), measure=True)
        try:
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            first = t.tick(snap, resident=True)
            assert last_order(t)[0] == (1 if view else 0)
            second = t.tick(snap, resident=True)
            outs.append((first, second, t.tick(snap)))
        finally:
            t.close()
    for a, b in zip(outs[0], outs[1]):
        assert_same(b, a)


@pytest.mark.parametrize("seed", range(40))
def test_the_view_equals_the_dense_scan_on_random_snapshots(seed, monkeypatch):
    from test_gpu_parity import random_env
    from hyperqueue_amd.tick import Tick

    env = random_env(seed)
    snap = env.snapshot()
    outs = []
    for view in ("0", "1"):
        monkeypatch.setenv("HQTICK_ORDERED_VIEW", view)
        t = Tick(env.config)
        try:
            outs.append(t.tick(snap))
        finally:
            t.close()
    assert_same(outs[1], outs[0])


def test_the_view_equals_the_dense_scan_on_a_reduced_c3_tick(monkeypatch):
    from hyperqueue_amd.tick import Tick

    snap = workloads.make("c3p", seed=2, n_tasks=50_000, n_workers=64)
    outs = []
    for view in ("0", "1"):
        monkeypatch.setenv("HQTICK_ORDERED_VIEW", view)
        t = Tick(abi.make_config(time_limit_s=60.0))
        try:
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            outs.append(t.tick(snap, resident=True))
            t.ready_consume_last()
            outs.append(t.tick(snap, resident=True))
        finally:
            t.close()
    assert_same(outs[2], outs[0])
    assert_same(outs[3], outs[1])


def queue_snapshot(base: abi.Snapshot, ids, prio, rq) -> abi.Snapshot:
    import dataclasses

    o = np.argsort(ids, kind="stable")
    return dataclasses.replace(base, task_id=np.asarray(ids, np.uint64)[o], task_priority=np.asarray(prio, np.uint64)[o], task_rq=np.asarray(rq, np.uint32)[o])


def test_a_resident_loop_across_the_cap(oracle):
    """ticks over a resident set of more than 4096 levels with consume, adds (merged and appended) and removes; the set crosses the cap both ways"""
    from hyperqueue_amd.tick import Tick

    snap = many_levels(4100, 1, 4300, 8, seed=9)
    ids, prio, rq = [snap.task_id.copy(), snap.task_priority.copy(), snap.task_rq.copy()]
    rng = np.random.default_rng(4)
    t = Tick(abi.make_config(time_limit_s=60.0), measure=True)
    try:
        t.upload_ready(ids, prio, rq, sorted_=True)
        next_id = int(ids.max()) + 1
        views = []
        for step in range(12):
            cur = queue_snapshot(snap, ids, prio, rq)
            got = t.tick(cur, resident=True)
            views.append(last_order(t)[0])
            assert_same(got, oracle.tick(cur))
            taken = np.asarray(sorted({r[0] for rs in got.records for r in rs}), np.uint64)
            t.ready_consume_last()
            if len(taken):
                keep = ~np.isin(ids, taken)
                ids, prio, rq = ids[keep], prio[keep], rq[keep]
            if step == 4:   # below the cap: remove most distinct priorities
                _, first = np.unique(prio, return_index=True)
                drop = ids[np.isin(np.arange(len(ids)), first[: len(first) - 100])]
                t.ready_remove(drop)
                keep = ~np.isin(ids, drop)
                ids, prio, rq = ids[keep], prio[keep], rq[keep]
            elif step == 7:  # back above the cap: an appended batch of fresh priorities
                n = 5000
                nid = np.arange(next_id, next_id + n, dtype=np.uint64); next_id += n
                npr = np.asarray([priority_from_user(100_000 + i) for i in range(n)], np.uint64)
                t.ready_add(nid, npr, np.zeros(n, np.uint32))
                ids, prio, rq = np.concatenate([ids, nid]), np.concatenate([prio, npr]), np.concatenate([rq, np.zeros(n, np.uint32)])
            elif step % 3 == 2:  # merged adds: ids between the resident ones
                gaps = np.setdiff1d(np.arange(1, int(ids.max())), ids)[:50].astype(np.uint64)
                if len(gaps):
                    gp = np.asarray([priority_from_user(int(v)) for v in rng.integers(0, 6000, len(gaps))], np.uint64)
                    t.ready_add(gaps, gp, np.zeros(len(gaps), np.uint32))
                    ids, prio, rq = np.concatenate([ids, gaps]), np.concatenate([prio, gp]), np.concatenate([rq, np.zeros(len(gaps), np.uint32)])
        assert 1 in views and 0 in views
    finally:
        t.close()


def test_a_query_beyond_the_dense_caps_equals_the_oracle(oracle):
    from hyperqueue_amd.tick import Tick

    snap = many_levels(5000, 1, 5200, 8, seed=1)
    fake_ids = np.arange(1000, 1004, dtype=np.uint32)
    fake_total = np.tile(snap.worker_total[0], (4, 1))
    want = oracle.query(snap, fake_ids, fake_total)
    t = Tick(abi.make_config(time_limit_s=60.0), measure=True)
    try:
        got = t.query(snap, fake_ids, fake_total)
        assert list(got[0]) == list(np.asarray(want[0], bool))
    finally:
        t.close()


def test_over_the_group_cap_with_fewer_than_4096_levels(oracle):
    """1100 levels x 16 requests = 17 600 groups: the dense scan's group cap, not its level cap, sends the tick to the view (one-shot and resident)"""
    from hyperqueue_amd.tick import Tick

    snap = many_levels(1100, 16, 20_000, 8, cpu_div=128, one_cpu=True)
    want = oracle.tick(snap)
    for resident in (False, True):
        t = Tick(abi.make_config(time_limit_s=60.0), measure=True)
        try:
            if resident:
                t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            got = t.tick(snap, resident=resident)
            on, runs, levels, _us = last_order(t)
            assert on == 1 and levels == 1100
            assert_same(got, want)
        finally:
            t.close()


@pytest.mark.parametrize("flags", [0, abi.HQTICK_FLAG_NO_TICK_CACHES])
def test_a_first_tick_on_a_heterogeneous_cluster(flags, oracle):
    """the first tick of a context with Q <= 16 launches the speculative dense scan, learns that there are more than 4096 levels and falls through to
    the view: the worker evaluation it then redoes is what the placement must read.  Workers with different free capacities make a misread visible."""
    from hyperqueue_amd.tick import Tick

    snap = many_levels(4500, 1, 5000, 32, seed=11)
    snap.worker_free = snap.worker_total.copy()
    for w in range(len(snap.worker_id)):
        snap.worker_free[w, 0] = snap.worker_total[w, 0] * (w % 4) // 4   # a quarter of the cluster busy, the rest a quarter .. three quarters free
        if w % 5 == 0:
            snap.worker_free[w, 1] = 0
    want = oracle.tick(snap)
    t = Tick(abi.make_config(time_limit_s=60.0, flags=flags), measure=True)
    try:
        t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
        for _ in range(2):
            got = t.tick(snap, resident=True)
            assert last_order(t)[0] == 1
            assert_same(got, want)
        assert any(len(r) for r in got.records) and not all(len(r) == len(got.records[0]) for r in got.records)
    finally:
        t.close()


def test_a_failed_consume_in_tick_on_the_view_puts_its_tasks_back():
    """CONSUME_IN_TICK on the view: a tick that fails after its selection (a record sink too small) leaves the set as it was; the next tick hands out what a
    fresh context hands out on the same set"""
    import dataclasses

    import torch

    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import HqTickError, Tick

    snap = many_levels(5000, 1, 6000, 16, seed=7)
    t = Tick(abi.make_config(time_limit_s=60.0, flags=abi.HQTICK_FLAG_CONSUME_IN_TICK), measure=True)
    ref = Tick(abi.make_config(time_limit_s=60.0))
    try:
        t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        lib = t._lib
        lib.hqtick_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        lib.hqtick_set_record_sink.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        assert lib.hqtick_set_shard(t._ctx, 0, 1) == 0
        W = len(snap.worker_id)
        small = torch.zeros(sink_layout(W, 4)[4], dtype=torch.uint8, device="cuda")
        assert lib.hqtick_set_record_sink(t._ctx, C.c_void_p(small.data_ptr()), C.c_size_t(small.numel())) == 0
        empty = dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))
        n0 = t.ready_count()
        with pytest.raises(HqTickError) as ei:
            t.tick(empty, resident=True)
        assert "back in the resident ready set" in str(ei.value)
        assert last_order(t)[0] == 1 and t.ready_count() == n0
        assert lib.hqtick_set_record_sink(t._ctx, None, 0) == 0
        got = t.tick(empty, resident=True)
        ref.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
        want = ref.tick(empty, resident=True)
        assert_same(got, want)
        handed = sum(len(r) for r in got.records)
        assert handed > 0 and t.ready_count() == n0 - handed
        # and what is left is exactly the set minus what was handed out: the next ticks agree as well
        ref.ready_consume_last()
        assert_same(t.tick(empty, resident=True), ref.tick(empty, resident=True))
    finally:
        t.close(); ref.close()


def test_a_resident_query_beyond_the_caps(oracle):
    """hqtick_query_resident beyond the census's caps: the answer is the oracle's, rq_ready the queue sizes, and the context is unchanged (its next tick is
    a fresh context's)"""
    import dataclasses

    from hyperqueue_amd.tick import Tick

    for n_levels, n_classes, div in ((5000, 1, 16), (1100, 16, 128)):
        snap = many_levels(n_levels, n_classes, 20_000 if n_classes > 1 else 5200, 8, seed=1, cpu_div=div, one_cpu=n_classes > 1)
        fake_ids = np.arange(1000, 1004, dtype=np.uint32)
        fake_total = np.tile(snap.worker_total[0], (4, 1))
        want_loaded, _ = oracle.query(snap, fake_ids, fake_total)
        t = Tick(abi.make_config(time_limit_s=60.0), measure=True)
        ref = Tick(abi.make_config(time_limit_s=60.0))
        try:
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            empty = dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))
            loaded, _opt, rq_ready = t.query_resident(empty, fake_ids, fake_total)
            assert list(loaded) == list(want_loaded)
            assert list(rq_ready) == np.bincount(snap.task_rq, minlength=n_classes).tolist()
            got = t.tick(empty, resident=True)
            ref.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            assert_same(got, ref.tick(empty, resident=True))
            want = oracle.tick(snap)
            # what the view decides — the batches — is the oracle's; the placement too wherever the answer is the canonical one (a coupled model of several
            # requests may stop at its certificate: test_gpu_parity.py's discovery test compares the same way)
            assert got.status == want.status and got.batches == want.batches
            if got.is_canonical:
                assert_same(got, want)
        finally:
            t.close(); ref.close()


def test_consume_after_a_blevel_update_on_a_comb_dag(oracle):
    """a 5000-node chain whose node i also waits for its own head task: after hqtick_graph_blevel(UPDATE_READY) the 5000 ready heads have 5000 distinct
    priorities.  The tick on them equals the oracle's on those priorities; a b-level update between the tick and hqtick_ready_consume_last (a new task
    behind one head raises its b-level) does not change what the consume takes out."""
    import dataclasses

    from hyperqueue_amd.tick import Tick

    K = 5000
    base = many_levels(1, 1, 10, 8)
    heads = np.arange(1, K + 1, dtype=np.uint64)
    chain = np.arange(K + 1, 2 * K + 1, dtype=np.uint64)
    ids = np.concatenate([heads, chain])
    deps = [[] for _ in range(K)] + [[int(heads[i])] + ([int(chain[i - 1])] if i else []) for i in range(K)]
    t = Tick(abi.make_config(time_limit_s=60.0), measure=True)
    try:
        t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        p0 = priority_from_user(0)
        ready = t.graph_add_tasks(ids, np.full(len(ids), p0, np.uint64), np.zeros(len(ids), np.uint32), deps)
        assert sorted(ready.tolist()) == heads.tolist()
        t.graph_blevel(update_ready=True)
        prio = t.graph_priorities(heads)
        assert len(np.unique(prio)) == K
        snap = dataclasses.replace(base, _keep=[], task_id=heads, task_priority=prio, task_rq=np.zeros(K, np.uint32))
        empty = dataclasses.replace(base, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))
        got = t.tick(empty, resident=True)
        assert last_order(t)[0] == 1
        assert_same(got, oracle.tick(snap))
        taken = {r[0] for rs in got.records for r in rs}
        assert taken
        # a chain of new tasks behind the LAST head (the lowest b-level before; none of them ready) lifts that head's b-level above every other, then the
        # consume of the tick's selection
        assert int(heads[-1]) not in taken
        t.graph_add_tasks(np.asarray([3 * K + j for j in range(1, 3 * K)], np.uint64), np.full(3 * K - 1, p0, np.uint64), np.zeros(3 * K - 1, np.uint32),
                          [[int(heads[-1])] if j == 1 else [3 * K + j - 1] for j in range(1, 3 * K)])
        t.graph_blevel(update_ready=True)
        assert t.graph_priorities(heads[-1:])[0] > prio.max()
        t.ready_consume_last()
        left = np.asarray(sorted(set(heads.tolist()) - taken), np.uint64)
        assert t.ready_count() == len(left)
        snap2 = dataclasses.replace(base, _keep=[], task_id=left, task_priority=t.graph_priorities(left), task_rq=np.zeros(len(left), np.uint32))
        assert_same(t.tick(empty, resident=True), oracle.tick(snap2))
    finally:
        t.close()
