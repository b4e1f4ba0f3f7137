"""Seams of the resident worker set (hqtick_cluster_*, hqtick_retracting_*) that test_gpu_cluster.py does not reach: request tables that outgrow
the device allocation followed by a membership change, every delta back to back on the one staging buffer (without and with the assignment ledger), a second
upload of a smaller worker set and a drop on one context, and the refusals with their codes and words.  The expected worker set is kept by `_Set` below, never
read back from the library; every tick runs with HQTICK_CHECK_CLUSTER=1 and is compared with a plain context's tick on the full snapshot of the same state."""
import dataclasses

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads
from test_gpu_cluster import _same, _tick

pytestmark = pytest.mark.gpu


class _Set:
    """the worker side of a snapshot as the host tracks it, changed by the same deltas the library is sent"""

    def __init__(self, snap):
        W, self.R, self.base = len(snap.worker_id), snap.n_resources, snap
        self.id = np.array(snap.worker_id, np.uint32)
        self.total = np.array(snap.worker_total, np.uint64).reshape(W, self.R).copy()
        self.free = np.array(snap.worker_free, np.uint64).reshape(W, self.R).copy()
        self.rem = np.array(snap.worker_remaining_ns, np.int64)
        self.flags = np.array(snap.worker_flags, np.uint8)
        self.blocked = {}  # worker id -> [(rq, variant)]

    def snap(self, base=None):
        W = len(self.id)
        blocked = [(w, q, v) for w, wid in enumerate(self.id.tolist()) for (q, v) in self.blocked.get(wid, [])]
        return dataclasses.replace(base or self.base, _keep=[], worker_id=self.id.copy(), worker_total=self.total.reshape(-1).copy(), worker_free=self.free.reshape(-1).copy(),
                                   worker_remaining_ns=self.rem.copy(), worker_min_utilization=np.zeros(W, np.float32), worker_flags=self.flags.copy(),
                                   worker_group=np.zeros(W, np.uint32), n_groups=1, blocked=blocked, assigned=[[] for _ in range(W)], prefilled=[[] for _ in range(W)])

    def update(self, t, rows, free, rem=None):
        self.free[rows] = free
        if rem is not None:
            self.rem[rows] = rem
        t.cluster_update_workers(rows, self.free[rows], rem)

    def add(self, t, ids, total, free, rem):
        t.cluster_add_workers(ids, total, free, remaining_ns=rem)
        self.id = np.concatenate([self.id, np.asarray(ids, np.uint32)]); self.total = np.concatenate([self.total, total]); self.free = np.concatenate([self.free, free])
        self.rem = np.concatenate([self.rem, np.asarray(rem, np.int64)]); self.flags = np.concatenate([self.flags, np.full(len(ids), abi.HQ_WORKER_SN, np.uint8)])

    def remove(self, t, ids):
        assert t.cluster_remove_workers(ids) == []  # (no Retracting task names these workers)
        keep = ~np.isin(self.id, ids)
        self.id, self.total, self.free, self.rem, self.flags = self.id[keep], self.total[keep], self.free[keep], self.rem[keep], self.flags[keep]
        for w in ids:
            self.blocked.pop(int(w), None)

    def set_blocked(self, t, wid, pairs):
        t.cluster_set_blocked(wid, pairs)
        self.blocked[wid] = list(pairs)

    def set_flags(self, t, ids, flags):
        t.cluster_set_flags(ids, flags)
        for w, f in zip(ids, flags):
            self.flags[self.id.tolist().index(w)] = f


def _ticks_equal(res, plain, snap):
    """the resident context on the snapshot with its worker arrays (the rows in HBM are checked against the test's own) and without them (the library's mirror
    completes it), both against the plain context"""
    want = plain.tick(snap)
    _same(res.tick(snap), want)
    _same(res.tick(snap, resident_workers=True), want)
    return want


def _refused(call, words):
    from hyperqueue_amd.tick import HqTickError

    with pytest.raises(HqTickError) as err:
        call()
    assert err.value.code == abi.HQTICK_E_INVALID and words in str(err.value), str(err.value)


# ---------------------------------------------------------------------------------------------- 1: the request tables outgrow the allocation, then the set changes
def _table_bytes(W, R, nv, ne):
    """worker rows [total W x R u64][free W x R u64][remaining W i64], then per entry amount u64 + resource u32 + kind u8, per variant min time u64 + entry offset u32
    (one offset more than variants), 64 bytes of slack"""
    return (2 * W * R + W) * 8 + ne * 13 + nv * 12 + 4 + 64


def test_request_tables_outgrow_the_allocation_then_the_set_changes():
    W, R, NV, PER = 8, 16, 420, 16
    w = workloads._uniform_workers(W, 1, [64.0] * R)
    ids, prio, _ = workloads._tasks(3000, [1.0], 0)
    one, two, three = [workloads._variant([(0, 1)])], [workloads._variant([(0, 2), (1, 1)])], [workloads._variant([(0, 1), (2, 0.5)])]
    small = abi.Snapshot(requests=[one], task_id=ids, task_priority=prio, task_rq=np.zeros(len(ids), np.uint32), **w)
    # two more small classes, then 14 classes of 30 variants that each ask for all 16 resources: 420 variants, 6720 entries.  Ready tasks of the first three only.
    wide = [[workloads._variant([(r, 0.25 * (1 + (q + v + r) % 7)) for r in range(PER)]) for v in range(30)] for q in range(NV // 30)]
    big = dataclasses.replace(small, _keep=[], requests=[one, two, three] + wide, task_rq=(np.arange(len(ids)) % 3).astype(np.uint32))
    nv, ne = 3 + NV, 5 + NV * PER
    first, second = _table_bytes(W, R, 1, 1), _table_bytes(W, R, nv, ne)
    assert second > 1.25 * (first + 65536) + 256          # beyond what the first upload allocated: the tick moves the worker rows to a new allocation
    assert 32 * R * 16 + 256 + ne * 13 + nv * 12 + 20 < 150 * 1024  # ... and still within what the worker evaluation stages in LDS
    plain, res = _tick(), _tick(HQTICK_CHECK_CLUSTER=1)
    try:
        st = _Set(small)
        res.cluster_upload(small)
        _ticks_equal(res, plain, small)
        assert sum(len(x) for x in _ticks_equal(res, plain, big).records) > 0
        st.remove(res, [int(st.id[2])])
        row = np.full((1, R), 48 * workloads.FR, np.uint64)
        st.add(res, [100], row, row // np.uint64(2), [abi.HQ_NO_TIME_LIMIT])
        st.update(res, [W - 1], row // np.uint64(4), [3_600_000_000_000])
        _ticks_equal(res, plain, st.snap(big))
        _ticks_equal(res, plain, st.snap(small))
    finally:
        plain.close(); res.close()


# ---------------------------------------------------------------------------------------------- 2: every delta back to back, one tick at the end
def _resident_tick(t, snap, ledger):
    sc = snap.to_c(resident_workers=True)
    if ledger:  # the ledger is the tick's source of running tasks: no assigned CSR
        sc.assigned_off = None; sc.assigned_rq = None; sc.assigned_variant = None
    return abi.parse_result(t.tick_raw(sc), len(snap.worker_id), snap.n_resources)


@pytest.mark.parametrize("ledger", [False, True])
def test_deltas_back_to_back(ledger):
    snap = workloads.make_steady("c3", seed=7, n_tasks=4000, n_workers=6)
    snap.assigned = [[] for _ in snap.worker_id]  # (the lowered free rows stay; with the ledger on they are what it was seeded with)
    plain, res = _tick(), _tick(HQTICK_CHECK_CLUSTER=1)
    try:
        st = _Set(snap)
        res.cluster_upload(snap)
        if ledger:
            res.assigned_enable([])
        SN = abi.HQ_WORKER_SN
        st.update(res, [0, 3], st.total[[0, 3]])
        st.add(res, [50], st.total[:1], st.total[:1] // np.uint64(2), [abi.HQ_NO_TIME_LIMIT])
        st.update(res, [6], st.total[6:7] // np.uint64(4), [7_200_000_000_000])
        st.remove(res, [int(st.id[2])])
        st.update(res, [2], st.total[2:3] // np.uint64(2))  # the row that moved up
        st.set_blocked(res, int(st.id[1]), [(0, 0), (3, 0)])
        st.set_flags(res, [int(st.id[4])], [SN | abi.HQ_WORKER_STOPPING])
        assert res.cluster_workers().tolist() == st.id.tolist() and res.cluster_worker_flags().tolist() == st.flags.tolist()
        if ledger:
            assert (res.assigned_free_rows() == st.free).all()
        cur = st.snap()
        want = plain.tick(cur)
        assert sum(len(x) for x in want.records) > 0
        _same(_resident_tick(res, cur, ledger), want)
        if not ledger:
            _same(res.tick(cur), want)
    finally:
        plain.close(); res.close()


# ---------------------------------------------------------------------------------------------- 3: a second upload of a smaller set, a drop
def test_re_upload_and_drop():
    eight = workloads.make_steady("c3", seed=2, n_tasks=3000, n_workers=8)
    four = workloads.make_steady("c3", seed=4, n_tasks=3000, n_workers=4)
    four.worker_id = np.array([3, 40, 41, 90], np.uint32)
    four.worker_total = np.asarray(four.worker_total, np.uint64) * np.uint64(2); four.worker_free = np.asarray(four.worker_free, np.uint64) + np.uint64(workloads.FR)
    plain, res = _tick(), _tick(HQTICK_CHECK_CLUSTER=1)
    try:
        res.retracting_add([11, 12], [1, 2])  # the Retracting table is no part of the worker set: uploads and the drop leave it alone
        res.cluster_upload(eight)
        assert res.retracting_count() == 2
        _ticks_equal(res, plain, eight)
        res.cluster_upload(four)  # the buffers do not shrink; the worker count follows
        assert res.retracting_count() == 2 and res.cluster_workers().tolist() == four.worker_id.tolist()
        _ticks_equal(res, plain, four)
        res.cluster_drop()
        assert res.retracting_count() == 2
        _refused(lambda: res.tick(four, resident_workers=True), "without a resident worker set")
        res.cluster_upload(eight)
        assert res.retracting_count() == 2
        _ticks_equal(res, plain, eight)
    finally:
        plain.close(); res.close()


# ---------------------------------------------------------------------------------------------- 4: refusals keep their code and words, and leave no partial state
def test_refusals_keep_their_code_and_words():
    snap = workloads.make_steady("c3", seed=9, n_tasks=3000, n_workers=5)
    R = snap.n_resources
    row = np.asarray(snap.worker_total, np.uint64).reshape(-1, R)[:1]
    top = int(snap.worker_id.max())
    plain, res = _tick(), _tick(HQTICK_CHECK_CLUSTER=1)
    try:
        for call in (lambda: res.cluster_update_workers([0], row), lambda: res.cluster_add_workers([top + 1], row), lambda: res.cluster_remove_workers([top]),
                     lambda: res.cluster_set_blocked(top, [(0, 0)]), lambda: res.cluster_set_flags([top], [abi.HQ_WORKER_SN])):
            _refused(call, "without hqtick_cluster_upload")
        _same(res.tick(snap), plain.tick(snap))
        res.cluster_upload(snap)
        fewer = dataclasses.replace(workloads.make_steady("c3", seed=9, n_tasks=3000, n_workers=4), _keep=[])

        def resident_retracting_without_ids():  # (asked of the plain context: a resident worker set would supply the ids)
            sc = snap.to_c(resident_workers=True)
            sc.n_workers = 0; sc.n_retracting = abi.HQ_RETRACTING_RESIDENT
            plain.tick_raw(sc)

        for call, words in ((lambda: res.cluster_add_workers([top], row), "ids must ascend"),
                            (lambda: res.cluster_add_workers([top + 2, top + 2], np.concatenate([row, row])), "ids must ascend"),
                            (lambda: res.cluster_remove_workers([top + 1]), "unknown (or repeated) worker id"),
                            (lambda: res.cluster_remove_workers([top, 1, top]), "unknown (or repeated) worker id"),
                            (lambda: res.cluster_set_flags([1, top], [abi.HQ_WORKER_SN, 0x80]), "undefined flag bits"),
                            (lambda: res.tick(fewer), "uploaded for another worker set"),
                            (resident_retracting_without_ids, "resident retracting table without worker ids")):
            _refused(call, words)
            _ticks_equal(res, plain, snap)  # nothing of the refused call stayed
            assert res.cluster_workers().tolist() == snap.worker_id.tolist() and res.cluster_worker_flags().tolist() == np.asarray(snap.worker_flags).tolist()
    finally:
        plain.close(); res.close()
