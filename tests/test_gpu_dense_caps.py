"""The dense (level, request) scan from 5 priority levels up to its caps (L <= 4096 levels, G = L * Q <= 16384 groups).

Level discovery (k_distinct_priorities, k_sort_levels), the group histogram (k_level_hist), the row scan (k_scan_rows / k_scan_rows_wg), the selection
(k_select) and the resident query's k_census all pick their code path from (L, Q, G).  Every shape below sits on one side of such a branch, next to its
neighbour on the other side.  What the kernels WRITE — the level table and the (level, request) histogram, read back through hqtick_debug_last_scan — is
compared with a plain numpy count (host_stages.scan_outputs), the variant that ran is asserted from the launch geometry the hook reports, and the tick's
answer is compared with the ordered view's (HQTICK_ORDERED_VIEW=1: none of these kernels) and with the canonical oracle's.  Everything is exact."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import host_stages
from hyperqueue_amd import abi, workloads
from hyperqueue_amd.core import priority_from_user
from test_gpu_many_levels import assert_same, last_order, many_levels, queue_snapshot

MAX_LEVELS, MAX_GROUPS, MAX_GROUPS_4W = 4096, 16384, 2048   # csrc/kernels.h
TOP = np.uint64(0xFFFFFFFFFFFFFFFF)                          # PRIO_EMPTY: the one priority the discovery's set cannot hold (k_sort_levels' `shift`)

# (L, Q, top) -> the branch the shape sits on
DENSE = [
    (4, 17, False),     # k_level_hist<4,true,1>: at most four levels (table in the kernel arguments) with G = 68 > 64 groups, one counter row per wavefront
    (2, 40, False),     # k_level_hist<4,true,1> again (G = 80), Q > 16: no speculative scan behind the discovery
    (4, 513, False),    # k_level_hist<1,true,1>: four levels, G = 2052 > MAX_GROUPS_4W — one wavefront per workgroup; k_select<1,2,1>
    (5, 1, False),      # just above the four-level variant: the speculative K1 refuses, k_level_hist<4,false,1> scans; k_select<4,0,16>
    (64, 1, False),     # G = 64: the last plan that travels in k_select<4,0,64>'s arguments
    (65, 1, False),     # G = 65: the first plan staged from HBM, k_select<4,1,1>; k_sort_levels pads 65 values to P = 128
    (512, 1, False),    # k_census: the level table staged in LDS (L = CENSUS_LDS_LEVELS)
    (513, 1, False),    # k_census: the level table searched in place (L > CENSUS_LDS_LEVELS); k_sort_levels pads to P = 1024
    (512, 8, False),    # k_census at G = CENSUS_LDS_BINS = 4096: the last LDS histogram, level table in LDS
    (513, 8, False),    # k_census with G = 4104 > CENSUS_LDS_BINS: every add goes to the global table, level table searched in place
    (1024, 2, False),   # k_level_hist<4,false,1> at G = 2048 = MAX_GROUPS_4W with the level table in LDS (L = 1024): 8 KB + 32 KB; k_select<4,1,1> with 64 KB of LDS (hipFuncSetAttribute)
    (1025, 1, False),   # the level table searched in HBM (lds_levels_for: L > 1024), still four wavefronts per workgroup
    (1025, 2, False),   # level table in HBM AND one wavefront per workgroup (G = 2050): k_level_hist<1,false,1>
    (2048, 1, False),   # G = 2048: the last four-wavefront table; k_select<4,1,1> through 2048 groups
    (2049, 1, False),   # G = 2049: the first one-wavefront table, k_level_hist<1,false,1> and k_select<1,2,1>
    (128, 16, False),   # G = 2048 with a short level table (L = 128 in LDS, Q = 16: the speculative scan runs first and refuses)
    (129, 16, False),   # G = 2064: one wavefront per workgroup with the level table in LDS
    (1024, 4, False),   # k_census at G = 4096 = CENSUS_LDS_BINS with L > CENSUS_LDS_LEVELS
    (1025, 4, False),   # k_census above its bins (G = 4100) and its level limit
    (4095, 1, False),   # just under the level cap: k_sort_levels with my_slot[4] not quite full, P = 4096
    (4096, 1, False),   # the level cap: k_sort_levels at n = 4096 exactly (my_slot[4] full, P = 4096, every bitonic step)
    (4096, 4, False),   # both caps at once: L = 4096, G = 16384; k_select<1,2,1> with 64 KB of LDS (hipFuncSetAttribute)
    (4095, 4, False),   # G = 16380: just under the group cap with the level table in HBM
    (1024, 16, False),  # the group cap with the level table in LDS: k_level_hist<1,false,1> needs 8 KB + 64 KB = 72 KB of LDS (hipFuncSetAttribute)
    (4095, 1, True),    # k_sort_levels' `shift` branch at the cap: 4095 values in the set + u64::MAX = 4096 levels
    (7, 3, True),       # `shift` on a small table (7 levels of which one is u64::MAX; P = 8 for 6 values)
    (4096, 1, True),    # `shift` onto the cap itself: 4095 values in the set + u64::MAX = 4096 levels, the last of them written to levels[4095] — still dense
]
# just over a cap: the tick lands on the ordered view and its answer is still right
VIEW = [
    (4097, 1, True),    # 4096 values in the set (k_sort_levels sorts a full table) + u64::MAX = 4097 levels: `shift` pushes the table over the level cap
    (4097, 1, False),   # one level too many: the discovery's compact list overflows
    (1024, 17, False),  # 17 408 groups with the level table in LDS
    (4096, 5, False),   # 20 480 groups at the level cap
]


def cluster_of(L: int, Q: int):
    """(n_workers, cpu_div of many_levels: 128 cpus / cpu_div per worker, busy) for a shape: the smallest departure from 8 workers x 8 cpus at which the canonical
    oracle answers a tick in about a second (shape_snapshot's docstring)"""
    if Q <= 3:
        return 8, 16, False
    if Q <= 5 or (L <= 4 and Q <= 40):
        return 8, 128, False
    return 1, 128, Q > 40


def shape_snapshot(L: int, Q: int, top: bool = False, seed: int = 0) -> abi.Snapshot:
    """dense_shape on the cluster the shape's placement allows.  The scan does not depend on the cluster; the placement does.  Up to three one-cpu classes the
    8 workers x 8 cpus place in milliseconds and the canonical oracle answers in about a second.  From four classes on, that cluster's model (Q batches of a
    level x 8 workers, all of equal weight) is one the product answers with a certified optimum that is not the canonical one, and the canonical oracle takes
    19 s at (1024, 4), 27 s at (4096, 4) and more than 100 s at Q >= 8.  So: Q = 4, 5 and the four-level shapes (4, 17), (2, 40) run on 8 workers x 1 cpu (oracle
    0.8-2.4 s), Q >= 8 on one worker with one cpu (oracle 0.7-0.9 s), and (4, 513) on one worker whose one cpu is busy: with a free cpu the oracle's tie-break
    over 2052 equal columns does not end within 100 s, with none it takes 0.7 s, and the 513 batches per level it compares are what the scan decides.  On every
    one of these clusters the product's answer is the canonical one, so every tick is compared with the oracle's in full."""
    n_workers, cpu_div, busy = cluster_of(L, Q)
    snap = dense_shape(L, Q, top=top, seed=seed, n_workers=n_workers, cpu_div=cpu_div)
    if busy:
        snap.worker_free = snap.worker_total.copy()
        snap.worker_free[:, 0] = 0
    return snap


def shape_id(s):
    return f"{s[0]}x{s[1]}" + ("top" if s[2] else "")


def dense_shape(L: int, Q: int, N: int = None, seed: int = 0, top: bool = False, n_workers: int = 8, cpu_div: int = 16) -> abi.Snapshot:
    """many_levels' cluster (by default 8 workers x 8 cpus; the tests go through shape_snapshot) with Q one-cpu request classes and a sorted-id ready set of exactly L distinct priorities in which
    every one of the L * Q (level, request) groups is nonempty: the first L * Q tasks enumerate the groups, the rest is random, then everything is shuffled.
    top: the highest of the L priorities is 2^64 - 1.  N defaults to L * Q + 777: no slice, tile or pair boundary falls on the end of the set."""
    G = L * Q
    N = G + 777 if N is None else N
    assert N >= G
    snap = many_levels(1, Q, N, n_workers, seed=seed, cpu_div=cpu_div, one_cpu=True)
    snap.requests = [[workloads._variant([(0, 1)])] for _ in range(Q)]
    rng = np.random.default_rng([L, Q, seed, int(top)])
    g = np.concatenate([np.arange(G, dtype=np.int64), rng.integers(0, G, N - G)])
    rng.shuffle(g)
    table = np.asarray([priority_from_user(p) for p in range(L)], np.uint64)   # ascending with p
    if top:
        table[L - 1] = TOP
    snap.task_priority = table[g // Q]
    snap.task_rq = (g % Q).astype(np.uint32)
    return snap


def numpy_scan(snap: abi.Snapshot):
    """(levels u64[L] descending, hist u32[L * Q]) by the plain count of tests/host_stages.py"""
    _f, _t, levels, hist = host_stages.scan_outputs(snap.to_c())
    return levels, hist


def last_scan(t, which: int):
    """hqtick_debug_last_scan -> None (the call did not run the dense table) or (L, G, shape[4], levels, hist)"""
    f = t._lib.hqtick_debug_last_scan
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), abi.u64p, C.c_uint32, abi.u32p, C.c_uint32]
    nl, ng, shape = C.c_uint32(0xDEAD), C.c_uint32(0xDEAD), (C.c_uint32 * 4)(7, 7, 7, 7)
    levels, hist = np.full(MAX_LEVELS, 0xABAB, np.uint64), np.full(MAX_GROUPS, 0xABAB, np.uint32)
    rc = f(t._ctx, which, C.byref(nl), C.byref(ng), shape, levels.ctypes.data_as(abi.u64p), len(levels), hist.ctypes.data_as(abi.u32p), len(hist))
    assert rc in (0, 1), rc
    if rc == 0:
        assert (nl.value, ng.value, list(shape)) == (0xDEAD, 0xDEAD, [7, 7, 7, 7]) and (levels == 0xABAB).all() and (hist == 0xABAB).all()   # nothing written
        return None
    assert nl.value <= MAX_LEVELS and ng.value <= MAX_GROUPS
    return nl.value, ng.value, list(shape), levels[: nl.value].copy(), hist[: ng.value].copy()


def check_scan(t, snap: abi.Snapshot, want_levels, want_hist, tasks_per_wave: int = 256):
    """the dense scan of t's last tick wrote numpy's level table and histogram, with the kernel variants its (L, G) calls for"""
    assert last_order(t)[0] == 0
    got = last_scan(t, 0)
    assert got is not None
    L, G, shape, levels, hist = got
    Q, N = len(snap.requests), len(snap.task_id)
    print(f"dense scan: L {L} G {G} shape {shape}")
    assert (L, G) == (len(want_levels), len(want_levels) * Q)
    assert (levels == want_levels).all()
    assert (hist == want_hist).all(), np.flatnonzero(hist != want_hist)[:10]
    assert shape[0] == (4 if G <= MAX_GROUPS_4W else 1)      # wavefronts per workgroup of K1 / K4
    assert shape[1] == tasks_per_wave and shape[2] == (N + tasks_per_wave - 1) // tasks_per_wave
    assert shape[3] == (1 if L <= 1024 else 0)               # level table on chip / searched in HBM
    return shape


def fake_workers(snap: abi.Snapshot):
    """the query's new workers: four like the cluster's; from eight classes on, one (four one-cpu workers x Q equal classes cost the oracle's query 1-3 s); at 513
    classes one without a cpu, which no task loads (with a cpu, the 513 equal columns cost the product's solver 5 s on the GPU box and the oracle's more than 100 s)"""
    Q = len(snap.requests)
    n = 4 if Q <= 5 else 1
    total = np.tile(snap.worker_total[0], (n, 1))
    if Q > 40:
        total[:, 0] = 0
    return np.arange(1000, 1000 + n, dtype=np.uint32), total


def free_cpus(snap: abi.Snapshot) -> int:
    return int(snap.worker_free[:, 0].sum()) // abi.HQ_FRACTIONS_PER_UNIT


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import Oracle

    return Oracle(abi.make_config(time_limit_s=60.0), canonical=True)


def new_tick(monkeypatch, view: bool, flags: int = 0):
    from hyperqueue_amd.tick import Tick

    monkeypatch.setenv("HQTICK_ORDERED_VIEW", "1" if view else "0")
    return Tick(abi.make_config(time_limit_s=60.0, flags=flags), measure=True)


# ---------------------------------------------------------------------------------------------- CPU checks of the test's own tools
@pytest.mark.parametrize("shape", DENSE + VIEW, ids=shape_id)
def test_the_generator_fills_every_group(shape):
    L, Q, top = shape
    snap = dense_shape(L, Q, top=top)
    assert len(snap.task_id) == L * Q + 777 and (np.diff(snap.task_id.astype(np.int64)) > 0).all() and len(snap.requests) == Q
    lv = np.unique(snap.task_priority)
    assert len(lv) == L and (lv[-1] == TOP) == top
    pairs = set(zip(snap.task_priority.tolist(), snap.task_rq.tolist()))
    assert len(pairs) == L * Q and snap.task_rq.max() == Q - 1
    assert (L <= MAX_LEVELS and L * Q <= MAX_GROUPS) == (shape in DENSE)


def test_the_numpy_count_equals_a_dictionary_count():
    snap = dense_shape(65, 3)
    levels, hist = numpy_scan(snap)
    count = {}
    for p, q in zip(snap.task_priority.tolist(), snap.task_rq.tolist()):
        count[(p, q)] = count.get((p, q), 0) + 1
    want_levels = sorted({p for p, _ in count}, reverse=True)
    assert levels.tolist() == want_levels and len(hist) == 65 * 3
    assert hist.tolist() == [count.get((p, q), 0) for p in want_levels for q in range(3)]
    assert int(hist.sum()) == len(snap.task_id)


# ---------------------------------------------------------------------------------------------- every dense shape
@pytest.mark.gpu
@pytest.mark.parametrize("shape", DENSE, ids=shape_id)
def test_a_dense_shape_counts_what_numpy_counts(shape, oracle, monkeypatch):
    """every dense shape on its cluster (shape_snapshot: 8 workers x 8 cpus up to three classes, smaller from four classes on, where the canonical oracle would take
    tens of seconds; the level table and the histogram are compared over all L x Q groups on any cluster, the tick reaches the top levels only)"""
    L, Q, top = shape
    snap = shape_snapshot(L, Q, top)
    levels, hist = numpy_scan(snap)
    assert len(levels) == L and len(hist) == L * Q and hist.min() >= 1
    want = oracle.tick(snap)
    fake_ids, fake_total = fake_workers(snap)
    want_loaded = oracle.query(snap, fake_ids, fake_total)[0]
    outs = {}
    for view in (False, True):
        one, res = new_tick(monkeypatch, view), new_tick(monkeypatch, view)
        try:
            outs[view, "one-shot"] = one.tick(snap)
            if not view:
                check_scan(one, snap, levels, hist)
                assert last_scan(one, 1) is None   # no query yet
            else:
                assert last_order(one)[0] == 1 and last_scan(one, 0) is None
            res.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            if not view:   # the census of the resident set, before any tick of this context
                loaded, _opt, rq_ready = res.query_resident(snap, fake_ids, fake_total)
                assert list(loaded) == list(np.asarray(want_loaded, bool))
                assert rq_ready.tolist() == np.bincount(snap.task_rq, minlength=Q).tolist()
                census = last_scan(res, 1)
                assert census is not None and last_scan(res, 0) is None
                assert (census[0], census[1], census[2]) == (L, L * Q, [0, 0, 0, 0])
                assert (census[3] == levels).all() and (census[4] == hist).all(), np.flatnonzero(census[4] != hist)[:10]
            outs[view, "resident"] = res.tick(snap, resident=True)   # (the queried context's next tick must be a fresh context's)
            if not view:
                check_scan(res, snap, levels, hist)
                again = res.tick(snap, resident=True)   # on the cached level table
                check_scan(res, snap, levels, hist)
                assert_same(again, outs[view, "resident"])
        finally:
            one.close(); res.close()
    for how in ("one-shot", "resident"):
        assert_same(outs[False, how], outs[True, how])
        assert sum(len(r) for r in outs[False, how].records) >= free_cpus(snap)   # the cluster is filled
        assert outs[False, how].is_canonical
        assert_same(outs[False, how], want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", VIEW, ids=shape_id)
def test_a_shape_just_over_a_cap_lands_on_the_view(shape, oracle, monkeypatch):
    """(on shape_snapshot's clusters: (4096, 5) on 8 workers x 1 cpu, (1024, 17) on one worker with one cpu, where the canonical oracle takes about a second)"""
    L, Q, top = shape
    snap = shape_snapshot(L, Q, top)
    want = oracle.tick(snap)
    fake_ids, fake_total = fake_workers(snap)
    want_loaded, _ = oracle.query(snap, fake_ids, fake_total)
    one, res = new_tick(monkeypatch, False), new_tick(monkeypatch, False)
    try:
        got = one.tick(snap)
        on, runs, n_levels, _us = last_order(one)
        assert on == 1 and n_levels == L and runs == L * Q and last_scan(one, 0) is None
        assert got.is_canonical
        assert_same(got, want)
        res.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
        loaded, _opt, rq_ready = res.query_resident(snap, fake_ids, fake_total)
        assert list(loaded) == list(np.asarray(want_loaded, bool))
        assert rq_ready.tolist() == np.bincount(snap.task_rq, minlength=Q).tolist()
        assert last_scan(res, 1) is None
        assert_same(res.tick(snap, resident=True), want)
        assert last_order(res)[0] == 1 and last_scan(res, 0) is None
    finally:
        one.close(); res.close()


# ---------------------------------------------------------------------------------------------- big sets: dense against the view and numpy only
@pytest.mark.gpu
@pytest.mark.parametrize("L,Q,what", [
    (4096, 4, "tasks_per_wave"),   # phase_a doubles tasks_per_wave to keep n_waves * G <= 2^24: G = 16384 with more than 262 144 tasks
    (4096, 1, "workgroup_scan"),   # k_scan_rows_wg (rows of more than 1024 slices) over 4096 rows
])
def test_a_big_set_on_the_dense_table(L, Q, what, monkeypatch):
    snap = dense_shape(L, Q, N=300_000)
    levels, hist = numpy_scan(snap)
    outs = []
    for view in (False, True):
        t = new_tick(monkeypatch, view)
        try:
            outs.append(t.tick(snap))
            if not view:
                tpw = 512 if what == "tasks_per_wave" else 256
                shape = check_scan(t, snap, levels, hist, tasks_per_wave=tpw)
                if what == "tasks_per_wave":
                    assert shape[1] == 512 and shape[2] * L * Q <= 1 << 24 < 2 * shape[2] * L * Q
                else:
                    assert shape[2] > 1024
        finally:
            t.close()
    assert_same(outs[0], outs[1])
    assert sum(len(r) for r in outs[0].records) == 64


# ---------------------------------------------------------------------------------------------- the selection through every group
@pytest.mark.gpu
@pytest.mark.parametrize("L", [2048, 4096])   # k_select<4,1,1> with 64 KB of LDS / k_select<1,2,1>: one request, so the placement separates and the solver stays trivial
def test_a_cluster_larger_than_the_set_takes_every_group(L, monkeypatch):
    n = L + 777
    snap = dense_shape(L, 1, n_workers=n // 128 + 2, cpu_div=1)   # workers of 128 one-cpu slots, more of them than N / 128
    assert int(snap.worker_total[:, 0].sum()) // abi.HQ_FRACTIONS_PER_UNIT > n
    levels, hist = numpy_scan(snap)
    outs = []
    for view in (False, True):
        t = new_tick(monkeypatch, view)
        try:
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            outs.append(t.tick(snap, resident=True))
            if not view:
                check_scan(t, snap, levels, hist)
        finally:
            t.close()
    assert_same(outs[0], outs[1])
    taken = sorted(r[0] for rs in outs[0].records for r in rs)
    assert taken == snap.task_id.tolist()


# ---------------------------------------------------------------------------------------------- tombstones and the cached level table
def stripped(snap: abi.Snapshot) -> abi.Snapshot:
    """the snapshot a resident host sends: no task columns"""
    return dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))


def without(snap: abi.Snapshot, result: abi.Result) -> abi.Snapshot:
    """the ready set of `snap` minus what `result` handed out"""
    taken = np.asarray(sorted(r[0] for rs in result.records for r in rs), np.uint64)
    assert len(taken) == 64   # 8 workers x 8 cpus
    keep = ~np.isin(snap.task_id, taken)
    return queue_snapshot(snap, snap.task_id[keep], snap.task_priority[keep], snap.task_rq[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("consume_in_tick", [False, True])
@pytest.mark.parametrize("L,Q", [(1025, 2), (4096, 4)])
def test_removed_levels_leave_the_dense_table(L, Q, consume_in_tick, monkeypatch):
    """A resident set after a tick's consume and the removal of every task of three levels.  The tick that follows still runs on the cached level table — phase_a
    keeps a table until a tick has SEEN an empty level in it —, in which the consumed and the removed levels are rows of zeros: its nonempty levels and their
    counts must be numpy's on the live set.  The tick after that has rediscovered the table: levels and histogram equal numpy's outright, the removed levels are
    gone (at (1025, 2) that takes the table back under 1024 levels and 2048 groups: the other variants of K1 and K4).  All three ticks equal the view's."""
    snap = dense_shape(L, Q)
    all_levels = np.unique(snap.task_priority)[::-1]
    gone = all_levels[[L // 3, L // 2 + 1, L - 1]]   # (below what a 64-cpu cluster reaches in two ticks)
    empty = stripped(snap)
    outs = []
    for view in (False, True):
        t = new_tick(monkeypatch, view, abi.HQTICK_FLAG_CONSUME_IN_TICK if consume_in_tick else 0)
        try:
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)
            first = t.tick(empty, resident=True)
            if not consume_in_tick:
                t.ready_consume_last()
            live = without(snap, first)
            drop = live.task_id[np.isin(live.task_priority, gone)]
            assert len(drop) >= 3 * Q and t.ready_remove(drop) == len(drop)
            keep = ~np.isin(live.task_priority, gone)
            live = queue_snapshot(live, live.task_id[keep], live.task_priority[keep], live.task_rq[keep])
            assert t.ready_count() == len(live.task_id)
            levels, hist = numpy_scan(live)
            assert len(levels) < L - 2 and not np.isin(gone, levels).any()
            second = t.tick(empty, resident=True)
            if not view:   # the cached table: L levels, of which the consumed and the removed ones are empty
                stale = last_scan(t, 0)
                assert stale is not None and last_order(t)[0] == 0 and (stale[0], stale[1]) == (L, L * Q) and (stale[3] == all_levels).all()
                rows = stale[4].reshape(L, Q)
                nonempty = rows.sum(axis=1) > 0
                assert (stale[3][nonempty] == levels).all() and (rows[nonempty].reshape(-1) == hist).all()
            if not consume_in_tick:
                t.ready_consume_last()
            live2 = without(live, second)
            assert t.ready_count() == len(live2.task_id)
            levels2, hist2 = numpy_scan(live2)
            third = t.tick(empty, resident=True)
            if not view:   # rediscovered: the live set's table, on the columns as uploaded (tombstones included) or compacted
                assert last_order(t)[0] == 0
                L3, G3, shape, got_levels, got_hist = last_scan(t, 0)
                print(f"dense scan after removes: L {L3} G {G3} shape {shape}")
                assert (L3, G3) == (len(levels2), len(levels2) * Q)
                assert (got_levels == levels2).all() and (got_hist == hist2).all()
                assert shape[0] == (4 if G3 <= MAX_GROUPS_4W else 1) and shape[3] == (1 if L3 <= 1024 else 0)
                assert shape[1] == 256 and shape[2] in ((len(snap.task_id) + 255) // 256, (len(live2.task_id) + 255) // 256)
            outs.append((first, second, third))
        finally:
            t.close()
    for a, b in zip(outs[0], outs[1]):
        assert_same(a, b)


# ---------------------------------------------------------------------------------------------- Retracting tasks deep in the one-wavefront table
@pytest.mark.gpu
@pytest.mark.parametrize("L,Q,seed", [(2049, 1, 6), (1024, 16, 3)])   # (seeds that put at least two tasks into the top level)
def test_retracting_tasks_deep_in_the_dense_table(L, Q, seed, oracle, monkeypatch):
    """five Retracting tasks — two in the top level, three in levels below the 1000th — whose queue positions k_rank_of reads from rows deep in the one-wavefront
    table (G > 2048).  Equal to the view's answer and to the canonical oracle's; (1024, 16) on one worker with one cpu (shape_snapshot: the oracle takes 35 s on
    8 workers x 1 cpu there, 0.7 s on one)."""
    snap = shape_snapshot(L, Q, seed=seed)
    levels, hist = numpy_scan(snap)
    order = np.lexsort((snap.task_id, ~snap.task_priority))   # priority descending, then id
    lvl_of = len(levels) - 1 - np.searchsorted(levels[::-1], snap.task_priority[order])   # index in the descending table
    top_two = order[lvl_of == 0][:2]
    assert len(top_two) == 2
    deep = [order[lvl_of == l][-1] for l in (1001, 1010, L - 1)]
    pick = np.sort(snap.task_id[np.concatenate([top_two, deep]).astype(np.int64)])
    snap.retracting = [(int(tid), i % len(snap.worker_id), abi.HQ_NO_WORKER, 0) for i, tid in enumerate(pick.tolist())]
    t, v = new_tick(monkeypatch, False), new_tick(monkeypatch, True)
    try:
        got = t.tick(snap)
        check_scan(t, snap, levels, hist)
        on_view = v.tick(snap)   # (positions from the view's inverse permutation, k_order_rank_of)
        assert last_order(v)[0] == 1
    finally:
        t.close(); v.close()
    assert_same(got, on_view)
    assert got.is_canonical
    assert_same(got, oracle.tick(snap))
