"""The ordered view of the ready set (csrc/order.hip) read back in full and compared, exactly, with numpy.

A tick on the view reads the head of every request's segment and nothing else; these tests build the view of a resident set by itself (hqtick_debug_order_view:
the same build_view a tick calls, on a sub-context of its own) and compare ALL of it — the permutation, its inverse, the level ranks, the run table, the digits
that got a pass — with order_cases.view_reference, then launch k_order_select and k_order_rank_of on it (hqtick_debug_order_select / _rank_of) against plain
definitions of theirs.  Every case names the branch or loop trip it sits on.  Every comparison is == on whole arrays."""
import contextlib
import functools

import numpy as np
import pytest

import order_cases as oc
from hyperqueue_amd import abi
from hyperqueue_amd.core import priority_from_user
from order_cases import TOMB, NONE64, ORDER_TILE

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def resident(ids, prio, rq, dead=None):
    """one context holding the set; yields (tick, the rq column as the device holds it)"""
    from hyperqueue_amd.tick import Tick

    t = Tick(abi.make_config(), measure=True)
    try:
        yield t, oc.load_set(t, ids, prio, rq, dead)
    finally:
        t.close()


def check_view(prio, rq, Q, dead=None, passes=None):
    """upload, remove, build, compare everything; returns the reference"""
    ids = oc.make_ids(len(rq))
    with resident(ids, prio, rq, dead) as (t, col):
        want = oc.view_reference(prio, col)
        rc, got = oc.order_view(t, Q, len(rq))
        assert rc == 0, t._err()
        if passes is not None:
            assert got.passes == passes
        oc.assert_view(got, want, col)
        assert t.ready_count() == want.n_live   # (the hook leaves the resident set alone)
    return want


# ---- tile and workgroup edges: random 64-bit priorities (all eight priority digits and rq byte 0 get a pass: 9 passes, an odd count), rq in [0, 5)
TILE_EDGES = [
    1,      # one slot: one tile, one lane; build_view's passes.empty() fallback (a single key is constant in every digit)
    63,     # one partial chunk of a wavefront
    64,     # exactly one chunk: the scatter's loop makes one trip with every lane active
    65,     # a second chunk with one active lane (the ballots run with 63 idle lanes)
    2047,   # one slot short of a tile
    2048,   # exactly one tile (ORDER_TILE)
    2049,   # a second tile holding one slot: k_radix_offsets scans two tile counts
    8192,   # four tiles = one full workgroup (WPB = 4)
    8193,   # a fifth tile in a second workgroup whose other three wavefronts return early
]


@pytest.mark.parametrize("n", TILE_EDGES)
def test_tile_and_workgroup_edges(n):
    prio, rq, Q = oc.random64(n, np.random.default_rng(n))
    want = check_view(prio, rq, Q)
    assert want.n_live == n


# ---- every digit alone, then together: which digits get a pass, in what number, and which pass is the last
DIGIT_SETS = [
    *[(dg,) for dg in range(12)],   # one pass on digit dg alone.  dg < 8: a byte of ~priority; 8: rq byte 0; 9-11: digit_of's `dg >= 8` arm with shifts 8, 16, 24
                                    # (rq = k << 8 | 3 with Q = 70 000; k << 16 | 3; {3, 0x01000003} with Q just above).  One pass: it writes d_perm directly.
    (2, 9),          # 2 passes (first writes d_perm2), the last on an rq digit: level_after = 0, the level ranks are read off d_perm2 before the last pass
    (1, 6),          # 2 passes, the last on a priority digit: level_after = the last pass
    (3, 7, 10),      # 3 passes (d_perm, d_perm2, d_perm), the last on rq byte 2
    (0, 4, 5),       # 3 passes, all on priority digits
    (0, 5, 8, 11),   # 4 passes, the last on rq byte 3
    (1, 2, 4, 7),    # 4 passes, all on priority digits (byte 7: the sign of a user priority)
    tuple(range(12)),  # all 12 digits vary: mask 0xFFF, 12 passes
]


@pytest.mark.parametrize("dgs", DIGIT_SETS, ids=lambda d: "d" + "_".join(map(str, d)))
def test_each_digit_and_their_combinations(dgs):
    prio, rq, Q = oc.digits_vary(list(dgs), 5000, np.random.default_rng(list(dgs)))
    if dgs == (9,):
        Q = 70_000
    check_view(prio, rq, Q, passes=sum(1 << d for d in dgs))


def test_all_live_keys_equal_with_tombstones():
    """no digit varies over the LIVE slots (the dead ones held other keys): passes.empty() pushes digit 0, whose one pass only drops the tombstones"""
    n = 5000
    rng = np.random.default_rng(7)
    prio, rq, Q = oc.random64(n, rng)
    dead = np.flatnonzero(rng.random(n) < 0.4)
    keep = np.setdiff1d(np.arange(n), dead)
    prio[keep], rq[keep] = np.uint64(0x0123456789ABCDEF), 2
    want = check_view(prio, rq, Q, dead=dead, passes=1)
    assert np.array_equal(want.perm, keep) and (want.n_runs, want.n_levels) == (1, 1)


# ---- key values
@pytest.mark.parametrize("family", ["edge_priorities", "user_edges", "user_with_blevels"])
def test_key_values(family):
    """edge_priorities: 0, 1, 2^63 - 1, 2^63, 2^64 - 1 (the complement's carries; PRIO_EMPTY is an ordinary key here).  user_edges: from_user_priority of -1, -2^31, 0,
    2^31 - 1 (byte 7 flips with the sign).  user_with_blevels: user priorities of both signs over b-levels in the low 32 bits (bytes 0-1 and 4-7 vary)."""
    prio, rq, Q = oc.FAMILIES[family](6001, np.random.default_rng(11))
    check_view(prio, rq, Q)


# ---- stability and lane patterns
def test_three_keys_over_100000_slots():
    """runs of equal keys through all 32 chunks of a tile and across 49 tiles: every position inside a run is the scatter's running counter + match-any rank"""
    prio, rq, Q = oc.few_keys(100_000, np.random.default_rng(3))
    want = check_view(prio, rq, Q)
    assert want.n_runs == 3


def test_a_tile_of_one_digit_value():
    """tile 1 (slots 2048..4095) holds one key: every ballot of its 32 chunks has 64 peers, one counter takes all 2048 positions"""
    n = 3 * ORDER_TILE + 100
    prio, rq, Q = oc.digits_vary([0, 8], n, np.random.default_rng(5))
    prio[ORDER_TILE:2 * ORDER_TILE], rq[ORDER_TILE:2 * ORDER_TILE] = prio[0], rq[0]
    check_view(prio, rq, Q, passes=0x101)


def test_chunks_of_64_distinct_digit_values():
    """every chunk of 64 consecutive slots holds 64 different values of the digit: match_any finds no peer, every lane is its counter's first"""
    n = 5000
    i = np.arange(n)
    byte = ((i % 64) * 4 + (i // 64) % 4).astype(np.uint64)
    prio = ~((np.uint64(oc.BASE_PRIO) & ~np.uint64(0xFF)) | byte)
    check_view(prio, np.full(n, 1, np.uint32), 5, passes=1)


@pytest.mark.parametrize("reverse", [False, True])
def test_sorted_and_reverse_sorted_sequences(reverse):
    """the slot order is already the view's order (every pass is the identity), or its reverse (every pass turns the tiles' order around)"""
    n = 10_000
    i = np.arange(n, dtype=np.uint64)
    rq = (np.arange(n) * 5 // n).astype(np.uint32)
    prio = np.uint64(1 << 40) - i * np.uint64(3)
    if reverse:
        prio, rq = prio[::-1].copy(), rq[::-1].copy()
    want = check_view(prio, rq, 5)
    assert np.array_equal(want.perm, np.arange(n)[::-1] if reverse else np.arange(n))


# ---- tombstones
def tomb_cases(name, n, rng):
    if name == "half":          # half of the slots dead, at random: every first-pass chunk has inactive lanes
        return np.flatnonzero(rng.random(n) < 0.5)
    if name == "two_tiles":     # slots 2048..6143 dead: tiles 1 and 2 count nothing, their scatter writes nothing
        return np.arange(2048, 6144)
    if name == "only_first":    # n_live = 1 at slot 0: the first pass covers 5 tiles of N slots, everything after it one tile of n = 1
        return np.arange(1, n)
    if name == "only_last":     # n_live = 1 at slot N - 1: the one live slot sits in the last, partial tile
        return np.arange(0, n - 1)
    if name == "all":           # n_live = 0: build_view returns after the histogram; no pass, no runs, no error
        return np.arange(n)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["half", "two_tiles", "only_first", "only_last", "all"])
def test_tombstones(name):
    n = 9000
    rng = np.random.default_rng(13)
    prio, rq, Q = oc.random64(n, rng)
    dead = tomb_cases(name, n, rng)
    want = check_view(prio, rq, Q, dead=dead)
    assert want.n_live == n - len(dead)
    if name == "all":
        assert (want.n_runs, want.n_levels, want.passes) == (0, 0, 0)


def test_a_request_id_beyond_Q_counts_only_where_it_is_live():
    n = 3000
    rng = np.random.default_rng(17)
    prio, rq, Q = oc.random64(n, rng)
    bad = np.sort(rng.choice(n, 40, replace=False))
    rq[bad] = rng.integers(Q, 1 << 31, len(bad)).astype(np.uint32)
    check_view(prio, rq, Q, dead=bad)                    # dead: the column holds the tombstone there, k_order_digits skips it before the check
    ids = oc.make_ids(n)
    with resident(ids, prio, rq, dead=bad[1:]) as (t, _col):   # one of them live
        rc, got = oc.order_view(t, Q, n)
        assert rc == abi.HQTICK_E_INVALID and got is None and "request id" in t._err()
        assert oc.order_rank_of(t, ids[:3])[0] == abi.HQTICK_E_INVALID   # no view was built


# ---- large sets: three varying digits (priority bytes 4-5, rq byte 0), up to 524 288 distinct (rq, priority) pairs
LARGE = [
    (524_288, 0.0),     # 256 tiles: k_radix_offsets' loop makes exactly one trip
    (524_289, 0.0),     # 257 tiles: a second trip that starts from s_carry (one tile in it)
    (600_001, 0.0),     # 293 tiles in every pass: the second trip scans 37 tiles
    (600_001, 0.2),     # a fifth removed: the first pass covers 293 tiles of N slots (two trips), the later ones 235 tiles of n live slots (one trip)
    (2_097_152, 0.0),   # n_live = 1024 tiles: k_run_scan's loop makes exactly one trip (in order_levels and in order_runs)
    (2_097_153, 0.0),   # 1025 tiles: k_run_scan's second trip, one tile, offset by the carry of > 100 000 run openings
    (2_200_003, 0.0),   # 1075 tiles: the second trip scans 51 tiles; k_radix_offsets makes five trips
]


@pytest.mark.parametrize("n,dead_share", LARGE, ids=lambda v: str(v))
def test_large_sets(n, dead_share):
    rng = np.random.default_rng(n)
    prio, rq, Q = oc.three_digits(n, rng)
    dead = np.flatnonzero(rng.random(n) < dead_share) if dead_share else None
    want = check_view(prio, rq, Q, dead=dead, passes=0x130)
    assert want.n_runs > (100_000 if n > 2_000_000 else 10_000)


# ---- determinism: what a sharded scheduler's replicas rest on
def test_two_contexts_build_the_same_bytes():
    n = 100_003
    rng = np.random.default_rng(19)
    prio, rq, Q = oc.user_with_blevels(n, rng, n_user=6, n_blevel=50)   # many equal keys: positions inside a run come from counters and ballots
    ids = oc.make_ids(n)
    views = []
    for _ in range(2):
        with resident(ids, prio, rq) as (t, _col):
            rc, got = oc.order_view(t, Q, n)
            assert rc == 0, t._err()
            views.append(got)
    a, b = views
    assert (a.n_live, a.n_runs, a.n_levels, a.passes) == (b.n_live, b.n_runs, b.n_levels, b.passes)
    for f in ("perm", "inv", "lrank", "run_rq", "run_start", "run_rank", "run_prio"):   # (no tombstones: inv and lrank are defined everywhere)
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


# ---- the hook leaves the context's ticks alone
@pytest.mark.parametrize("view", ["1", "0"])
def test_the_view_hook_does_not_touch_the_ticks_around_it(view, monkeypatch):
    """tick, hook, tick, consume, hook, tick == tick, tick, consume, tick on a context that never called the hook: the results of every tick, and what
    hqtick_debug_last_order reports after every step.  HQTICK_ORDERED_VIEW=1: the ticks use d_perm and a pending order_select themselves; 0: the dense scan
    with its cached level table (levels_valid)."""
    from hyperqueue_amd.tick import Tick
    from test_gpu_many_levels import assert_same, last_order, many_levels

    monkeypatch.setenv("HQTICK_ORDERED_VIEW", view)
    snap = many_levels(70, 8, 3000, 4, seed=5)   # 70 levels x 8 request classes on 4 small workers: 560 groups, dense unless the view is forced
    Q, N = len(snap.requests), len(snap.task_id)

    def run(hook: bool):
        t = Tick(abi.make_config(time_limit_s=20.0), measure=True)
        out = []
        try:
            t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq, sorted_=True)

            def step():
                if hook:
                    before = last_order(t)
                    rc, got = oc.order_view(t, Q, N)
                    assert rc == 0 and got.n_live == t.ready_count()
                    assert last_order(t) == before
            out.append(t.tick(snap, resident=True)); out.append(last_order(t)[:3])
            step()
            out.append(t.tick(snap, resident=True)); out.append(last_order(t)[:3])
            step()
            t.ready_consume_last()
            step()
            out.append(t.tick(snap, resident=True)); out.append(last_order(t)[:3])
            out.append(t.ready_count())
        finally:
            t.close()
        return out

    plain, hooked = run(False), run(True)
    assert plain[1][0] == int(view)
    for a, b in zip(plain, hooked):
        if isinstance(a, abi.Result):
            assert_same(b, a)
        else:
            assert b == a


# ---- selection: 30 000 slots, 40 requests, ~2900 runs
SEL_N, SEL_Q, SEL_EMPTY, SEL_MANY = 30_000, 40, (17, 39), 5   # requests 17 and 39 have no task (no run); request 5 has 150 priority levels (> 100 runs), the others 75


@functools.lru_cache(maxsize=None)
def sel_set():
    rng = np.random.default_rng(29)
    rq = rng.choice(np.setdiff1d(np.arange(SEL_Q), SEL_EMPTY), SEL_N).astype(np.uint32)
    level = np.where(rq == SEL_MANY, rng.integers(0, 150, SEL_N), rng.integers(0, 75, SEL_N))
    prio = np.asarray([priority_from_user(p) for p in range(150)], np.uint64)[level]
    dead = np.flatnonzero(rng.random(SEL_N) < 0.1)
    ids = oc.make_ids(SEL_N)
    col = rq.copy(); col[dead] = TOMB
    want = oc.view_reference(prio, col)
    for a in (ids, prio, rq, dead, col, want.perm, want.lrank, want.run_rq, want.run_start):
        a.setflags(write=False)
    return ids, prio, rq, dead, col, want, np.bincount(col[col != TOMB], minlength=SEL_Q)


def plan_of(take, tnc=None):
    take = np.asarray(take, np.int64)
    return np.concatenate([[0], np.cumsum(take)]), np.zeros(SEL_Q, np.int64) if tnc is None else np.asarray(tnc, np.int64), int(take.sum())


def random_plan(seed, have):
    rng = np.random.default_rng(seed)
    take = np.minimum(have, rng.integers(0, 60, SEL_Q))
    take[rng.random(SEL_Q) < 0.3] = 0
    tnc = np.zeros(SEL_Q, np.int64)
    for q in np.flatnonzero(take >= 2):
        if rng.random() < 0.5:
            nw = int(rng.integers(1, take[q] + 1))
            tnc[q] = nw << 16 | int(take[q]) // nw
    return plan_of(take, tnc)


def sel_plans():
    have = sel_set()[6]
    z = np.zeros(SEL_Q, np.int64)

    def one(**kv):
        take, tnc = z.copy(), z.copy()
        for q, v in kv.items():
            take[int(q[1:])], tnc[int(q[1:])] = v if isinstance(v, tuple) else (v, 0)
        return plan_of(take, tnc)
    spread = lambda total: plan_of(np.bincount(np.arange(total) % 7 * 5 + 1, minlength=SEL_Q))   # requests 1, 6, 11, ..., 31
    return {
        "random0": random_plan(0, have), "random1": random_plan(1, have), "random2": random_plan(2, have),
        "nothing_at_the_front": one(q2=9, q3=4),                # requests 0 and 1 share base 0 with request 2: the search must land on the LAST of them
        "nothing_in_the_middle": one(q0=5, q1=3, q8=6),         # requests 2-7 share request 8's base
        "nothing_at_the_end": one(q0=5, q20=7),                 # requests 21-39 share base n_sel: no j reaches them
        "a_whole_segment": one(q9=int(have[9])),                # position seg_end - 1 is the last one the guard lets through
        "across_100_runs": one(q5=int(have[5]), q6=10),         # request 5 has 150 runs: the run search goes 8 levels deep
        "one_worker": one(q3=(24, 1 << 16 | 24), q4=5),         # nw = 1: sw = p, dst = base + p — the identity in worker-major form
        "one_task_each": one(q3=(24, 24 << 16 | 1)),            # c = 1: sw = 0 for every p
        "grid_equals_take": one(q3=(24, 4 << 16 | 6), q4=3),    # nw * c = take: every position is transposed
        "grid_below_take": one(q3=(24, 4 << 16 | 5), q4=3),     # nw * c = 20 < 24: positions 20-23 keep dst = j
        "grid_above_take": one(q3=(23, 4 << 16 | 6), q4=3),     # nw * c = 24 > 23: p < nw * c always; only the cell (worker 3, task 5) = offset 23 stays empty
        "n_sel_1": one(q11=1), "n_sel_255": spread(255), "n_sel_256": spread(256), "n_sel_257": spread(257),   # one lane; one workgroup less a lane, exactly, and a second one with one lane
    }


@pytest.mark.parametrize("name", ["random0", "random1", "random2", "nothing_at_the_front", "nothing_in_the_middle", "nothing_at_the_end", "a_whole_segment", "across_100_runs",
                                  "one_worker", "one_task_each", "grid_equals_take", "grid_below_take", "grid_above_take", "n_sel_1", "n_sel_255", "n_sel_256", "n_sel_257"])
def test_selection_on_the_view(name):
    ids, prio, rq, dead, col, want, _have = sel_set()
    base, tnc, n_sel = sel_plans()[name]
    w_task, w_rank, _slots, w_err = oc.select_reference(ids, want, base, tnc, n_sel)
    assert w_err == 0 and (w_task != NONE64).all()
    with resident(ids, prio, rq, dead) as (t, _c):
        rc, got = oc.order_view(t, SEL_Q, SEL_N)
        assert rc == 0, t._err()
        oc.assert_view(got, want, col)
        rc, task, rank, after, err = oc.order_select(t, base, tnc, n_sel, 0, SEL_N)
        assert rc == 0, t._err()
        assert err == 0 and np.array_equal(task, w_task) and np.array_equal(rank, w_rank)
        assert np.array_equal(after, col)   # mode 0 marks nothing


def test_selection_mark_modes():
    """consume writes RQ_TOMBSTONE at exactly the selected slots and selects nothing; restore writes the request ids back; mark_and_select does both at once;
    none of them reaches the resident column"""
    ids, prio, rq, dead, col, want, have = sel_set()
    base, tnc, n_sel = random_plan(3, have)
    w_task, w_rank, slots, _ = oc.select_reference(ids, want, base, tnc, n_sel)
    consumed = col.copy(); consumed[slots] = TOMB
    assert len(slots) == n_sel and (col[slots] != TOMB).all()
    with resident(ids, prio, rq, dead) as (t, _c):
        assert oc.order_view(t, SEL_Q, SEL_N)[0] == 0
        assert oc.order_select(t, base, tnc, n_sel, 2, SEL_N)[0] == abi.HQTICK_E_INVALID   # restore needs the copy a consume left
        rc, task, rank, after, err = oc.order_select(t, base, tnc, n_sel, 1, SEL_N)        # consume
        assert (rc, err) == (0, 0) and np.array_equal(after, consumed)
        assert (task == NONE64).all() and (rank == TOMB).all()                              # ... selects nothing
        rc, task, rank, after, err = oc.order_select(t, base, tnc, n_sel, 2, SEL_N)        # restore, on the consumed copy
        assert (rc, err) == (0, 0) and np.array_equal(after, col)
        assert (task == NONE64).all() and (rank == TOMB).all()
        rc, task, rank, after, err = oc.order_select(t, base, tnc, n_sel, 3, SEL_N)        # mark_and_select
        assert (rc, err) == (0, 0) and np.array_equal(after, consumed)
        assert np.array_equal(task, w_task) and np.array_equal(rank, w_rank)
        assert t.ready_count() == want.n_live
        rc, again = oc.order_view(t, SEL_Q, SEL_N)                                          # the resident column is as it was
        assert rc == 0
        oc.assert_view(again, want, col)


@pytest.mark.parametrize("guard", ["one_more_than_the_segment", "a_request_without_runs"])
def test_selection_guards(guard):
    """the two early exits of k_order_select (in-bounds returns, not faults): err = 1, the j in question is not written, every other j is right"""
    ids, prio, rq, dead, col, want, have = sel_set()
    take = np.minimum(have, 20)
    if guard == "one_more_than_the_segment":
        take[9] = have[9] + 1                  # pos = seg_end for the last j of request 9
        n_bad = 1
    else:
        take[17] = 3                           # run_off[17] == run_off[18]: r0 >= r1 for three j
        n_bad = 3
    base, tnc, n_sel = plan_of(take)
    w_task, w_rank, _slots, w_err = oc.select_reference(ids, want, base, tnc, n_sel)
    assert w_err == 1 and (w_task == NONE64).sum() == n_bad
    with resident(ids, prio, rq, dead) as (t, _c):
        assert oc.order_view(t, SEL_Q, SEL_N)[0] == 0
        rc, task, rank, _after, err = oc.order_select(t, base, tnc, n_sel, 0, SEL_N)
        assert rc == 0, t._err()
        assert err == 1 and np.array_equal(task, w_task) and np.array_equal(rank, w_rank)


def test_the_select_hook_refuses_a_destination_outside_its_request():
    ids, prio, rq, dead, _col, _want, _have = sel_set()
    take = np.zeros(SEL_Q, np.int64); take[3], take[4] = 5, 5
    tnc = np.zeros(SEL_Q, np.int64); tnc[3] = 4 << 16 | 2     # position 3 -> worker 3, task 0 -> offset 6 >= 5
    base, tnc, n_sel = plan_of(take, tnc)
    with resident(ids, prio, rq, dead) as (t, _c):
        assert oc.order_view(t, SEL_Q, SEL_N)[0] == 0
        assert oc.order_select(t, base, tnc, n_sel, 0, SEL_N)[0] == abi.HQTICK_E_INVALID


# ---- rank_of
@pytest.mark.parametrize("n_want", [1, 256, 257])   # one lane; exactly one workgroup; a second workgroup with one lane
def test_rank_of(n_want):
    n = 5000
    rng = np.random.default_rng(31)
    prio, rq, Q = oc.user_with_blevels(n, rng)
    ids = oc.make_ids(n)
    dead = np.sort(rng.choice(np.setdiff1d(np.arange(1, n - 1), [77]), 700, replace=False))   # (the first id, the last one and ids[77] stay live)
    fixed = [ids[0], ids[-1],           # the first and the last id: the search ends at lo = 0 and lo = N - 1
             0, ids[0] - 1,             # below the smallest: lo = 0, ids[0] != id
             ids[-1] + 1, NONE64,       # above the largest: lo = N, nothing is read there
             ids[10] + 1, ids[4000] + 2,  # in the gaps between two ids
             ids[dead[0]], ids[dead[-1]],  # tombstoned: found, but not live
             ids[77], ids[77]]          # twice in one request
    want = np.asarray([int(x) for x in fixed], np.uint64) if n_want > 1 else ids[-1:].copy()
    if n_want > 1:
        fill = rng.integers(0, int(ids[-1]) + 5, n_want - len(want)).astype(np.uint64)
        want = np.concatenate([want, fill])
    with resident(ids, prio, rq, dead) as (t, col):
        ref = oc.view_reference(prio, col)
        rc, got = oc.order_view(t, Q, n)
        assert rc == 0, t._err()
        oc.assert_view(got, ref, col)
        w_rq, w_pos = oc.rank_of_reference(ids, col, ref, want)
        rc, g_rq, g_pos = oc.order_rank_of(t, want)
        assert rc == 0, t._err()
        assert np.array_equal(g_rq, w_rq) and np.array_equal(g_pos, w_pos)
        if n_want > 1:
            assert (w_rq[:2] != TOMB).all() and (w_rq[2:10] == TOMB).all() and w_rq[10] == w_rq[11] != TOMB
