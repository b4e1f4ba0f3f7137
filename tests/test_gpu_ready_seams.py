"""Two seams of the resident ready set's host side (hqtick_ready_*) that the scenario tests cross without pinning them: what a refused batch says and leaves
behind on each of the paths a batch can take, and the two edges of the rule that decides when the set compacts."""
import dataclasses

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads

pytestmark = pytest.mark.gpu

N0 = 64            # tasks resident before the batch
LOW = 1            # ids LOW, LOW + 1, ...: job 0, below every id of the workload (job 1, task 1..n) and none of them resident
DUPLICATE = "hqtick_ready_add: a task id is already in the ready set"
UNSORTED = "hqtick_ready_add: ids not strictly ascending"
RESERVED = "hqtick_ready_add: request id 0xFFFFFFFF is reserved"


def _bad_batch(path, refusal, ids):
    """ids and request ids of a batch of 2-3 tasks that takes `path` and is refused for `refusal`.  What decides the path is the batch's first and last id against
    the resident maximum: first above it and last not below first -> appended at the tail; first below it -> merged; nothing resident -> it becomes the set."""
    top = int(ids[-1]) if len(ids) else 0
    if path == "merge":
        bad = {"duplicate": [LOW, int(ids[5])], "unsorted": [LOW + 2, LOW + 1, LOW + 3], "reserved": [LOW, LOW + 1]}[refusal]
    else:  # the duplicate sits in the middle: the batch's first and last id still lie above everything resident
        bad = {"duplicate": [top + 1, top, top + 2], "unsorted": [top + 1, top + 3, top + 2, top + 4], "reserved": [top + 1, top + 2]}[refusal]
    rq = np.zeros(len(bad), np.uint32)
    if refusal == "reserved":
        rq[1] = 0xFFFFFFFF
    return np.asarray(bad, np.uint64), rq


# (path, refusal) -> the library's text, as the library before hqready::ReadySet produced it.  An appended batch's first id lies above the resident maximum, so a resident id
# inside it is also a step down: the append kernels report the order.  Nothing can be a duplicate on an empty set.
REFUSALS = [
    ("append", "duplicate", UNSORTED), ("append", "unsorted", UNSORTED), ("append", "reserved", RESERVED),
    ("append_packed", "duplicate", UNSORTED), ("append_packed", "unsorted", UNSORTED), ("append_packed", "reserved", RESERVED),
    ("merge", "duplicate", DUPLICATE), ("merge", "unsorted", UNSORTED), ("merge", "reserved", RESERVED),
    ("empty", "unsorted", UNSORTED), ("empty", "reserved", RESERVED),
]


@pytest.mark.parametrize("path,refusal,text", REFUSALS, ids=[f"{p}-{r}" for p, r, _ in REFUSALS])
def test_a_refused_batch_says_why_and_leaves_the_set(path, refusal, text):
    from hyperqueue_amd.tick import HqTickError, Tick

    snap = workloads.make("c3", n_tasks=N0, n_workers=4)
    n0 = 0 if path == "empty" else N0
    ids, p0 = snap.task_id[:n0], int(snap.task_priority[0])
    t = Tick(abi.make_config())
    t.upload_ready(ids, snap.task_priority[:n0], snap.task_rq[:n0])
    bad, rq = _bad_batch(path, refusal, ids)
    appends = t.kernel_stats()["ready_appends"]
    with pytest.raises(HqTickError) as e:
        if path == "append_packed":  # (the reserved request id through the u16 column: 0xFFFF)
            t.ready_add_packed([(int(i), 1) for i in bad], [(p0, len(bad))], rq.astype(np.uint16))
        else:
            t.ready_add(bad, np.full(len(bad), p0, np.uint64), rq)
    print(f"{path}-{refusal}: {e.value}")
    assert e.value.code == abi.HQTICK_E_INVALID
    assert str(e.value) == f"hqtick error {abi.HQTICK_E_INVALID}: {text}"
    assert t.ready_count() == n0 and t.kernel_stats()["ready_appends"] == appends
    # a good fresh batch right after it: appended — onto an empty set the first one becomes the set (no append counted), the one after it is appended
    fresh = np.uint64(max(int(bad.max()), int(ids[-1]) if n0 else 0) + 1) + np.arange(4, dtype=np.uint64)
    t.ready_add(fresh, np.full(4, p0, np.uint64), np.zeros(4, np.uint32))
    if path == "empty":
        assert t.ready_count() == 4 and t.kernel_stats()["ready_appends"] == appends
        fresh = fresh + np.uint64(4)
        t.ready_add(fresh, np.full(4, p0, np.uint64), np.zeros(4, np.uint32))
        n0 = 4
    assert t.ready_count() == n0 + 4 and t.kernel_stats()["ready_appends"] == appends + 1
    t.close()


# The set compacts when it holds more than 4096 rows and fewer than half of them are live.  Observed through ready_appends: a compaction leaves
# live + max(live, 4096) rows of room, so 3000 fresh ids fit behind the columns and are appended (+1); an uploaded column has only its buffer's slack
# (bytes + bytes / 4 + 256 B for bytes = 8 n + 8 of the id column), so the same batch does not fit and is merged (+0):
#   upload 8192: (8192 * 8 + 8) * 5 / 4 + 256 = 82186 B -> (82186 - 8) / 8 = 10272 rows < 8192 + 3000
#   upload 4096: (4096 * 8 + 8) * 5 / 4 + 256 = 41226 B -> (41226 - 8) / 8 =  5152 rows < 4096 + 3000   (8194 and 4097 rows, uncompacted, fall short the same way)
#   compacted to 2048 live: room for 2048 + 4096 = 6144 rows >= 2048 + 3000;  compacted to 4096 live: room for 8192 rows >= 4096 + 3000
EDGES = [(4097, 2049, True), (4096, 2049, False), (8194, 4098, True), (8192, 4096, False)]
BATCH = 3000


@pytest.mark.parametrize("n,k,compacts", EDGES, ids=[f"{n}-{k}" for n, k, _ in EDGES])
def test_compaction_rule_edges(n, k, compacts):
    from hyperqueue_amd.tick import Tick
    from oracle.oracle import Oracle

    cfg = abi.make_config(time_limit_s=20.0)
    snap = workloads.make("c3", n_tasks=n, n_workers=4)
    ids, prio, rq = snap.task_id.copy(), snap.task_priority.copy(), snap.task_rq.copy()
    t = Tick(cfg)  # (a fresh context: the alternate columns are unallocated)
    t.upload_ready(ids, prio, rq)
    assert t.ready_remove(ids[:k]) == k
    t.ready_consume_last()  # no tick pending: compacts if due, and only then
    assert t.ready_count() == n - k
    new_ids = ids[-1] + np.uint64(1) + np.arange(BATCH, dtype=np.uint64)
    new_prio, new_rq = np.full(BATCH, int(prio[0]), np.uint64), (np.arange(BATCH) % 8).astype(np.uint32)
    before = t.kernel_stats()["ready_appends"]
    t.ready_add(new_ids, new_prio, new_rq)
    took_append = t.kernel_stats()["ready_appends"] - before
    print(f"upload {n}, remove {k}: live {n - k}, ready_appends +{took_append}")
    assert took_append == (1 if compacts else 0)
    ids, prio, rq = np.concatenate([ids[k:], new_ids]), np.concatenate([prio[k:], new_prio]), np.concatenate([rq[k:], new_rq])
    assert t.ready_count() == len(ids)
    empty = dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))
    got = t.tick(empty, resident=True)
    want = Oracle(cfg, canonical=True).tick(dataclasses.replace(snap, _keep=[], task_id=ids, task_priority=prio, task_rq=rq))
    assert got.status == want.status and got.batches == want.batches and got.counts == want.counts
    assert got.records == want.records and got.retracts == want.retracts and (got.new_free == want.new_free).all()
    t.close()
