"""The ordered view of the ready set (csrc/order.hip) in plain numpy, the key families its tests draw from, and the ctypes side of the view
hooks of include/hqtick_debug.h.

The view has a plain definition: the live slots of the id-sorted columns ordered by (request ascending, priority descending, slot ascending), the inverse of
that permutation, the number of distinct priorities above every live slot's, and one row per nonempty (request, priority) pair.  Everything here is exact;
tests/test_order_reference.py checks these functions against sorted() with tuple keys on a machine without a GPU."""
import ctypes as C
import dataclasses

import numpy as np

from hyperqueue_amd import abi
from hyperqueue_amd.core import priority_from_user

TOMB = 0xFFFFFFFF          # csrc/kernels.h: RQ_TOMBSTONE; also what the hooks report for "not a live task" and leave where nothing was written
NONE64 = 0xFFFFFFFFFFFFFFFF
ORDER_TILE = 2048          # csrc/kernels.h: slots one wavefront ranks per pass


# ------------------------------------------------------------------------------------------------------ the reference
@dataclasses.dataclass
class View:
    n_live: int
    n_runs: int
    n_levels: int
    passes: int             # bit dg: digit dg got a radix pass
    perm: np.ndarray        # [n_live] u32
    inv: np.ndarray         # [N] u32, defined at live slots
    lrank: np.ndarray       # [N] u32, defined at live slots
    run_rq: np.ndarray
    run_start: np.ndarray
    run_rank: np.ndarray
    run_prio: np.ndarray    # u64


def pass_mask(prio: np.ndarray, rq: np.ndarray) -> int:
    """build_view's passes: every 8-bit digit of (rq, ~priority) that is not constant over the live slots; none at all: digit 0 (one pass still drops the tombstones)"""
    live = rq != TOMB
    if not live.any():
        return 0
    p, r = (~prio[live]).astype(np.uint64), rq[live].astype(np.uint32)
    mask = 0
    for dg in range(8):
        b = (p >> np.uint64(8 * dg)) & np.uint64(0xFF)
        mask |= int(b.min() != b.max()) << dg
    for dg in range(4):
        b = (r >> np.uint32(8 * dg)) & np.uint32(0xFF)
        mask |= int(b.min() != b.max()) << (8 + dg)
    return mask or 1


def view_reference(prio: np.ndarray, rq: np.ndarray) -> View:
    """prio u64 [N], rq u32 [N] with TOMB at dead slots"""
    prio, rq = np.asarray(prio, np.uint64), np.asarray(rq, np.uint32)
    N = len(rq)
    live = np.flatnonzero(rq != TOMB)
    perm = live[np.lexsort((live, ~prio[live], rq[live]))]   # rq ascending, priority descending, slot ascending
    n = len(perm)
    inv = np.full(N, TOMB, np.uint32)
    inv[perm] = np.arange(n, dtype=np.uint32)
    asc = np.unique(prio[live])
    lrank = np.full(N, TOMB, np.uint32)
    lrank[live] = (len(asc) - 1 - np.searchsorted(asc, prio[live])).astype(np.uint32)   # distinct priorities above the slot's
    k, p = rq[perm], prio[perm]
    opens = np.ones(n, bool)
    opens[1:] = (k[1:] != k[:-1]) | (p[1:] != p[:-1])
    start = np.flatnonzero(opens)
    return View(n, len(start), len(asc), pass_mask(prio, rq), perm.astype(np.uint32), inv, lrank, k[start].astype(np.uint32), start.astype(np.uint32),
                lrank[perm[start]].astype(np.uint32), p[start].astype(np.uint64))


def select_reference(ids: np.ndarray, view: View, rq_sel_base, q_tnc, n_sel: int):
    """k_order_select: (sel_task [n_sel] u64, sel_rank [n_sel] u32, selected slots [<= n_sel], err).  A j whose position lies outside its request's segment (or
    whose request has no run) is not written (NONE64 / TOMB stay) and sets err."""
    base, tnc = np.asarray(rq_sel_base, np.int64), np.asarray(q_tnc, np.int64)
    Q = len(tnc)
    seg = np.searchsorted(view.run_rq, np.arange(Q + 1))                       # runs of request q: [seg[q], seg[q + 1])
    seg_start = np.append(view.run_start, view.n_live).astype(np.int64)[seg]     # positions of request q: [seg_start[q], seg_start[q + 1])
    j = np.arange(n_sel, dtype=np.int64)
    q = np.searchsorted(base[:Q], j, side="right") - 1                          # the last request with rq_sel_base[q] <= j
    p = j - base[q]
    pos = seg_start[q] + p
    ok = (seg[q] < seg[q + 1]) & (pos < seg_start[q + 1])
    nw, c = tnc[q] >> 16, tnc[q] & 0xFFFF
    sw = p // np.maximum(nw, 1)
    major = (tnc[q] != 0) & (p < nw * c)
    dst = np.where(major, base[q] + (p - sw * nw) * c + sw, j)
    sel_task, sel_rank = np.full(n_sel, NONE64, np.uint64), np.full(n_sel, TOMB, np.uint32)
    slots = view.perm[pos[ok]]
    assert len(np.unique(dst[ok])) == ok.sum(), "the plan sends two tasks to one destination"
    sel_task[dst[ok]] = ids[slots]
    sel_rank[dst[ok]] = view.lrank[slots]
    return sel_task, sel_rank, slots, int(not ok.all())


def rank_of_reference(ids: np.ndarray, rq: np.ndarray, view: View, want):
    """k_order_rank_of: (request, position in the view) per wanted id; TOMB twice for an id that is absent or tombstoned"""
    want = np.asarray(want, np.uint64)
    lo = np.searchsorted(ids, want)
    at = np.minimum(lo, len(ids) - 1)
    found = (lo < len(ids)) & (ids[at] == want) & (rq[at] != TOMB)
    return np.where(found, rq[at], TOMB).astype(np.uint32), np.where(found, view.inv[at], TOMB).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------ key families
BASE_PRIO = 0x5AA5C33C0FF096E7   # what the constant bytes of ~priority are drawn from: no byte of it is 0x00 or 0xFF


def digits_vary(dgs, n: int, rng):
    """(prio, rq, Q) in which exactly the digits `dgs` of the sort key (0-7: bytes of ~priority, 8-11: bytes of rq) vary over the n slots.  rq byte 3 takes the
    values 0 and 1 and rq byte 2 four values, so that Q stays at or below 0x0103FFFF + 1."""
    key, rq = np.full(n, BASE_PRIO, np.uint64), np.zeros(n, np.uint32)
    if 8 not in dgs:
        rq |= np.uint32(3)
    for dg in dgs:
        hi = 256 if dg < 10 else (4 if dg == 10 else 2)
        b = rng.integers(0, hi, n)
        b[:hi] = np.arange(hi)[: len(b[:hi])]   # every value occurs (n >= 256 in every use; smaller sets take what fits)
        rng.shuffle(b)
        if dg < 8:
            key = (key & ~np.uint64(0xFF << (8 * dg))) | (b.astype(np.uint64) << np.uint64(8 * dg))
        else:
            rq |= b.astype(np.uint32) << np.uint32(8 * (dg - 8))
    return ~key, rq, int(rq.max()) + 1 if n else 1


def random64(n: int, rng, Q: int = 5):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.integers(0, Q, n).astype(np.uint32), Q


def edge_priorities(n: int, rng, Q: int = 5):
    vals = np.asarray([0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], np.uint64)
    return vals[rng.integers(0, len(vals), n)], rng.integers(0, Q, n).astype(np.uint32), Q


def user_edges(n: int, rng, Q: int = 5):
    """Priority::from_user_priority of the ends of i32 and their neighbours at zero: byte 7 of the key flips with the sign"""
    vals = np.asarray([priority_from_user(p) for p in (-1, -(1 << 31), 0, (1 << 31) - 1)], np.uint64)
    return vals[rng.integers(0, len(vals), n)], rng.integers(0, Q, n).astype(np.uint32), Q


def user_with_blevels(n: int, rng, Q: int = 5, n_user: int = 40, n_blevel: int = 700):
    """user priorities (both signs) in the high half, b-levels (hqtick_graph_blevel) in the low 32 bits"""
    user = rng.integers(-n_user // 2, n_user // 2, n)
    hi = np.asarray([priority_from_user(int(p)) for p in range(-n_user // 2, n_user // 2)], np.uint64)[user + n_user // 2]
    return hi | rng.integers(0, n_blevel, n).astype(np.uint64), rng.integers(0, Q, n).astype(np.uint32), Q


def few_keys(n: int, rng, n_keys: int = 3, Q: int = 5):
    """n_keys distinct (rq, priority) pairs: long runs of equal keys"""
    kp = rng.integers(0, 1 << 64, n_keys, dtype=np.uint64)
    kq = rng.integers(0, Q, n_keys).astype(np.uint32)
    pick = rng.integers(0, n_keys, n)
    return kp[pick], kq[pick], Q


def three_digits(n: int, rng, Q: int = 8):
    """the large sets: 65536 user priorities (bytes 4 and 5 of the key) x Q < 256 requests (rq byte 0) — three passes, up to 65536 * Q runs"""
    return (rng.integers(0, 1 << 16, n).astype(np.uint64) ^ np.uint64(0x80000000)) << np.uint64(32), rng.integers(0, Q, n).astype(np.uint32), Q


FAMILIES = {"random64": random64, "edge_priorities": edge_priorities, "user_edges": user_edges, "user_with_blevels": user_with_blevels, "few_keys": few_keys,
            "three_digits": three_digits}


def make_ids(n: int) -> np.ndarray:
    """ascending task ids with gaps (rank_of asks for ids that fall between them)"""
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)


# ------------------------------------------------------------------------------------------------------ the hooks
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def _p(a, t):
    return a.ctypes.data_as(t)


def load_set(t, ids, prio, rq, dead=None):
    """the resident set of Tick t: sorted upload, then hqtick_ready_remove of the ids at `dead` (the upload refuses 0xFFFFFFFF); returns the rq column as the device holds it"""
    rq = np.ascontiguousarray(rq, np.uint32)
    t.upload_ready(ids, prio, rq, sorted_=True)
    col = rq.copy()
    if dead is not None and len(dead):
        assert t.ready_remove(ids[dead]) == len(dead)
        col[dead] = TOMB
    return col


def order_view(t, Q: int, N: int):
    """hqtick_debug_order_view -> (rc, View or None)"""
    f = t._lib.hqtick_debug_order_view
    f.argtypes = [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u32p, C.c_uint64, u32p, u32p, u32p, u64p, C.c_uint32]
    f.restype = C.c_int
    counts = np.zeros(4, np.uint32)
    cap = max(N, 1)
    perm, inv, lrank, r_rq, r_st, r_rk = (np.full(cap, 0xA5A5A5A5, np.uint32) for _ in range(6))
    r_pr = np.zeros(cap, np.uint64)
    rc = f(t._ctx, Q, _p(counts, u32p), _p(perm, u32p), _p(inv, u32p), _p(lrank, u32p), cap, _p(r_rq, u32p), _p(r_st, u32p), _p(r_rk, u32p), _p(r_pr, u64p), cap)
    if rc:
        return rc, None
    n, nr = int(counts[0]), int(counts[1])
    return 0, View(n, nr, int(counts[2]), int(counts[3]), perm[:n], inv[:N], lrank[:N], r_rq[:nr], r_st[:nr], r_rk[:nr], r_pr[:nr])


def order_select(t, rq_sel_base, q_tnc, n_sel: int, mode: int, N: int):
    """hqtick_debug_order_select -> (rc, sel_task, sel_rank, rq_after, err)"""
    f = t._lib.hqtick_debug_order_select
    f.argtypes = [C.c_void_p, u32p, u32p, C.c_uint32, C.c_int, u64p, u32p, u32p, u32p]
    f.restype = C.c_int
    base, tnc = np.ascontiguousarray(rq_sel_base, np.uint32), np.ascontiguousarray(q_tnc, np.uint32)
    sel_task, sel_rank, after, err = np.zeros(max(n_sel, 1), np.uint64), np.zeros(max(n_sel, 1), np.uint32), np.zeros(max(N, 1), np.uint32), np.zeros(1, np.uint32)
    rc = f(t._ctx, _p(base, u32p), _p(tnc, u32p), n_sel, mode, _p(sel_task, u64p), _p(sel_rank, u32p), _p(after, u32p), _p(err, u32p))
    return rc, sel_task[:n_sel], sel_rank[:n_sel], after[:N], int(err[0])


def order_rank_of(t, want):
    f = t._lib.hqtick_debug_order_rank_of
    f.argtypes = [C.c_void_p, u64p, C.c_uint32, u32p, u32p]
    f.restype = C.c_int
    want = np.ascontiguousarray(want, np.uint64)
    out_rq, out_pos = np.zeros(len(want), np.uint32), np.zeros(len(want), np.uint32)
    rc = f(t._ctx, _p(want, u64p), len(want), _p(out_rq, u32p), _p(out_pos, u32p))
    return rc, out_rq, out_pos


def assert_view(got: View, want: View, rq: np.ndarray):
    """every array of the view, exactly; inv and lrank at the live slots (the kernels write nothing at a tombstone)"""
    live = rq != TOMB
    assert (got.n_live, got.n_runs, got.n_levels) == (want.n_live, want.n_runs, want.n_levels)
    assert got.passes == want.passes
    assert np.array_equal(got.perm, want.perm)
    assert np.array_equal(got.inv[live], want.inv[live])
    assert np.array_equal(got.lrank[live], want.lrank[live])
    assert np.array_equal(got.run_rq, want.run_rq)
    assert np.array_equal(got.run_start, want.run_start)
    assert np.array_equal(got.run_rank, want.run_rank)
    assert np.array_equal(got.run_prio, want.run_prio)
