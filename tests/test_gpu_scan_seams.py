"""A seam of phase A (the scan of the ready set, hqscan::Scanner) that the scenario tests do not cross: a ready set that holds a request id >= n_requests.  Every
scan kernel flags it without writing out of bounds (K1, the view's digit histogram, the census) and the library refuses the call from three places with one text.
Pinned on each path a scan can take: what the refusal says, that it leaves the resident set as it was, and that the context answers like a fresh one again once the
bad task is gone."""
import dataclasses

import numpy as np
import pytest

from hyperqueue_amd import abi, workloads

pytestmark = pytest.mark.gpu

N0 = 64
TEXT = "ready set holds a request id >= n_requests"
CASES = ["dense-first", "dense-first-no-spec", "dense-cached", "view", "census"]


def _with_ready(snap, ids, prio, rq):
    return dataclasses.replace(snap, _keep=[], task_id=np.asarray(ids, np.uint64), task_priority=np.asarray(prio, np.uint64), task_rq=np.asarray(rq, np.uint32))


def _same_tick(got, want):
    assert got.status == want.status and got.batches == want.batches and got.counts == want.counts
    assert got.records == want.records and got.retracts == want.retracts and (got.new_free == want.new_free).all()


def _fakes(R):
    ids = np.arange(1 << 20, (1 << 20) + 3, dtype=np.uint32)
    tot = np.zeros((3, R), np.uint64); tot[:, 0] = 16 * abi.HQ_FRACTIONS_PER_UNIT
    return ids, tot


@pytest.mark.parametrize("case", CASES)
def test_a_request_id_out_of_range_is_refused_and_the_set_recovers(case, monkeypatch):
    from hyperqueue_amd.tick import HqTickError, Tick
    from oracle.oracle import Oracle

    if case == "dense-first-no-spec":
        monkeypatch.setenv("HQTICK_NO_SPEC_SCAN", "1")
    if case == "view":
        monkeypatch.setenv("HQTICK_ORDERED_VIEW", "1")
    cfg = abi.make_config(time_limit_s=20.0)
    snap = workloads.make("c3", n_tasks=N0, n_workers=4)
    Q = len(snap.requests)
    assert 4 * Q <= 64  # a fresh context takes the speculative scan
    ids, prio, rq = snap.task_id.copy(), snap.task_priority.copy(), snap.task_rq.copy()
    empty = _with_ready(snap, [], [], [])
    t = Tick(cfg)  # (created under the case's environment: the two switches are read once per context)
    if case == "dense-cached":  # a good tick leaves its level table behind; the bad task arrives as a delta
        t.upload_ready(ids, prio, rq)
        first = t.tick(empty, resident=True)
        _same_tick(first, Oracle(cfg, canonical=True).tick(snap))
        t.ready_consume_last()
        taken = {int(task) for w in first.records for (task, _, _) in w}
        keep = np.asarray([int(i) not in taken for i in ids], bool)
        ids, prio, rq = ids[keep], prio[keep], rq[keep]
        assert t.ready_count() == len(ids)
        bad = int(snap.task_id[-1]) + 1  # ... in one batch with eight good ones, so that the tick after the recovery has something to place
        fresh = np.uint64(bad) + np.arange(9, dtype=np.uint64)
        fresh_rq = np.concatenate([[Q], np.arange(8) % Q]).astype(np.uint32)
        t.ready_add(fresh, np.full(9, int(snap.task_priority[0]), np.uint64), fresh_rq)
        ids, prio, rq = np.concatenate([ids, fresh[1:]]), np.concatenate([prio, np.full(8, int(snap.task_priority[0]), np.uint64)]), np.concatenate([rq, fresh_rq[1:]])
    else:
        bad = int(ids[17])
        rq_bad = rq.copy(); rq_bad[17] = Q
        t.upload_ready(ids, prio, rq_bad)
        keep = ids != np.uint64(bad)
        ids, prio, rq = ids[keep], prio[keep], rq[keep]
    n_before = t.ready_count()
    assert n_before == len(ids) + 1
    fake_ids, fake_tot = _fakes(snap.n_resources)
    with pytest.raises(HqTickError) as e:
        if case == "census":
            t.query_resident(empty, fake_ids, fake_tot)
        else:
            t.tick(empty, resident=True)
    print(f"{case}: {e.value}; live {n_before} -> {t.ready_count()}, {len(ids)} good tasks")
    assert e.value.code == abi.HQTICK_E_INVALID
    assert str(e.value) == f"hqtick error {abi.HQTICK_E_INVALID}: {TEXT}"
    assert t.ready_count() == n_before
    # the bad task leaves: the same context answers as if it had never been there
    assert t.ready_remove(np.asarray([bad], np.uint64)) == 1
    good = _with_ready(snap, ids, prio, rq)
    if case == "census":
        loaded, optimal, rq_ready = t.query_resident(empty, fake_ids, fake_tot)
        want_loaded, want_optimal = Tick(cfg).query(good, fake_ids, fake_tot)
        print(f"{case}: recovered, loaded {loaded.astype(int).tolist()} optimal {optimal} rq_ready {rq_ready.tolist()}")
        assert (loaded == want_loaded).all() and optimal == want_optimal
        assert (rq_ready == np.bincount(rq.astype(np.int64), minlength=Q).astype(np.uint64)).all()
    else:
        got = t.tick(empty, resident=True)
        print(f"{case}: recovered, status {got.status}, {sum(len(w) for w in got.records)} records")
        _same_tick(got, Oracle(cfg, canonical=True).tick(good))
    t.close()
