"""Seams of the mapping's host side (the plan and GPU phase C) that the scenario tests cross without pinning them: the replay of a tick's selection — as tombstones
(hqtick_ready_consume_last) and as the put-back of a failed HQTICK_FLAG_CONSUME_IN_TICK tick — on the dense scan and on the ordered view; an early round-robin
sweep left in flight by a tick that failed; the tick without any sweep launch and the reordering path; the three record forms of one placement; the sink of an
empty tick.  Small on purpose (at most 8 workers, 4 requests, 64 ready tasks): every result is compared with the canonical oracle's."""
import dataclasses

import numpy as np
import pytest

from hyperqueue_amd import abi
from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB

pytestmark = pytest.mark.gpu

SINK_MAGIC = 0x48515354
UNEQUAL = [1, 2, 4]     # cpus per worker: one key with the counts 1, 2, 4 — not worker-major, so K5a goes out early, right behind the key tables
UNIFORM = [4, 4, 4, 4]  # every worker takes 4 tasks of the one request: the key is stored worker-major and no sweep is launched at all


def _cfg(flags=0, fill_max=2):
    return abi.make_config(reserve=0, fill_max=fill_max, time_limit_s=20.0, flags=flags)


def _env(cfg, worker_cpus, n_tasks, two_requests=True, priority=0):
    e = SchedEnv(cfg)
    for c in worker_cpus:
        e.new_worker(WB(c))
    for i in range(n_tasks):
        e.new_task(TB().cpus(2 if two_requests and i % 5 == 4 else 1).user_priority(priority))
    return e


def _tick(cfg, monkeypatch, view):
    from hyperqueue_amd.tick import Tick

    if view:
        monkeypatch.setenv("HQTICK_ORDERED_VIEW", "1")  # (read when the context is created)
    return Tick(cfg)


def _oracle(cfg):
    from oracle.oracle import Oracle

    return Oracle(abi.make_config(reserve=cfg.proactive_filling_reserve, fill_max=cfg.proactive_filling_max, time_limit_s=20.0), canonical=True)


def _empty(snap):
    return dataclasses.replace(snap, _keep=[], task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))


def _without(snap, res):
    """the snapshot with the tasks `res` handed out gone from its ready set (the workers as they were)"""
    taken = np.asarray(sorted(t for recs in res.records for (t, _v, _k) in recs), np.uint64)
    keep = ~np.isin(snap.task_id, taken)
    return dataclasses.replace(snap, _keep=[], task_id=snap.task_id[keep], task_priority=snap.task_priority[keep], task_rq=snap.task_rq[keep]), len(taken)


def _same(got, want):
    assert got.status == want.status and got.is_optimal == want.is_optimal and got.batches == want.batches and got.counts == want.counts
    assert got.records == want.records and got.retracts == want.retracts and (got.new_free == want.new_free).all()
    assert sorted(zip(got.redirects, got.redirect_kinds)) == sorted(zip(want.redirects, want.redirect_kinds))


def _small_sink(W, n_records):
    import torch

    from hyperqueue_amd.sharded import sink_layout

    return torch.zeros(sink_layout(W, n_records)[4], dtype=torch.uint8, device="cuda:0")


@pytest.mark.parametrize("view", [False, True], ids=["dense", "view"])
def test_two_call_tick_replays_its_selection_as_tombstones(view, monkeypatch):
    """hqtick_run_resident, then hqtick_ready_consume_last: the selection once more, writing tombstones — the next tick equals the oracle's on what is left"""
    cfg = _cfg()
    snap = _env(cfg, UNEQUAL, 40).snapshot()
    o, t = _oracle(cfg), _tick(cfg, monkeypatch, view)
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    got = t.tick(_empty(snap), resident=True)
    _same(got, o.tick(snap))
    assert t.ready_count() == 40  # nothing is consumed before the second call
    t.ready_consume_last()
    left, n_taken = _without(snap, got)
    print(f"two-call, {'view' if view else 'dense'}: {n_taken} handed out, {t.ready_count()} left")
    assert n_taken > 0 and t.ready_count() == 40 - n_taken
    got2 = t.tick(_empty(snap), resident=True)
    _same(got2, o.tick(left))
    assert sum(len(r) for r in got2.records) > 0
    t.close()


@pytest.mark.parametrize("view", [False, True], ids=["dense", "view"])
def test_failed_consume_in_tick_puts_its_selection_back(view, monkeypatch):
    """HQTICK_FLAG_CONSUME_IN_TICK with a record sink too small for the tick: the refusal is a host-side check behind K4, whose tombstones the restore takes back.
    The tick has unequal counts per worker, so its K5a went out early and is still in flight when the sink check refuses."""
    from hyperqueue_amd.tick import HqTickError

    cfg = _cfg(abi.HQTICK_FLAG_CONSUME_IN_TICK)
    snap = _env(cfg, UNEQUAL, 40).snapshot()
    W = len(snap.worker_id)
    o, t = _oracle(cfg), _tick(cfg, monkeypatch, view)
    t.upload_ready(snap.task_id, snap.task_priority, snap.task_rq)
    small = _small_sink(W, 2)
    t.set_record_sink(small)
    with pytest.raises(HqTickError) as ei:
        t.tick(_empty(snap), resident=True)
    print(f"failed consume-in-tick, {'view' if view else 'dense'}: {ei.value}")
    assert ei.value.code == abi.HQTICK_E_CAPACITY and "record sink too small for this tick" in str(ei.value)
    assert "is back in the resident ready set" in str(ei.value)
    assert t.ready_count() == 40
    t.set_record_sink(None)
    got = t.tick(_empty(snap), resident=True)
    _same(got, o.tick(snap))
    _left, n_taken = _without(snap, got)
    assert n_taken > 0 and t.ready_count() == 40 - n_taken
    t.close()


def test_failed_tick_leaves_its_early_sweep_in_flight():
    """a plain tick whose keys have unequal counts per worker (K5a launched right behind the key tables) and whose sink is too small: the refusal leaves that launch
    uncovered by any wait.  The following tick, on the same tables, still equals the oracle's."""
    from hyperqueue_amd.tick import HqTickError, Tick

    cfg = _cfg()
    snap = _env(cfg, UNEQUAL, 24).snapshot()
    t = Tick(cfg)
    small = _small_sink(len(snap.worker_id), 2)
    t.set_record_sink(small)
    with pytest.raises(HqTickError) as ei:
        t.tick(snap)
    print(f"failed tick: {ei.value}")
    assert ei.value.code == abi.HQTICK_E_CAPACITY and str(ei.value) == f"hqtick error {abi.HQTICK_E_CAPACITY}: record sink too small for this tick"
    t.set_record_sink(None)
    got = t.tick(snap)
    _same(got, _oracle(cfg).tick(snap))
    assert t.kernel_stats()["sweep_us"] > 0  # this tick's own sweep ran
    t.close()


def test_uniform_tick_then_the_reordering_path():
    """a tick whose every key is stored worker-major (no sweep launch: on a fresh context the sweep's event pair was never recorded, its time stays 0), then — after
    that placement and its prefill sets are applied, some tasks finish and tasks of a lower priority arrive — a tick with a two-level queue and a prefill set, which needs the
    mapping kernel's stable sort"""
    from hyperqueue_amd.tick import Tick

    cfg = _cfg()
    e = _env(cfg, UNIFORM, 40, two_requests=False, priority=3)
    o, t = _oracle(cfg), Tick(cfg)
    snap = e.snapshot()
    got = t.tick(snap)
    want = o.tick(snap)
    _same(got, want)
    kinds = [k for recs in got.records for (_t, _v, k) in recs]
    print(f"uniform: {kinds.count(abi.HQ_REC_ASSIGN)} assigned, {kinds.count(abi.HQ_REC_PREFILL)} prefilled, sweep_us {t.kernel_stats()['sweep_us']}")
    assert kinds.count(abi.HQ_REC_ASSIGN) == 16 and kinds.count(abi.HQ_REC_PREFILL) > 0
    assert t.kernel_stats()["sweep_us"] == 0
    e.apply(want)
    done = 0
    for task in sorted(e.tasks.values(), key=lambda x: x.id):
        if task.state == 1 and done < 6:
            e.finish_task(task.id, task.worker); done += 1
    for _ in range(5):
        e.new_task(TB().cpus(1).user_priority(0))
    snap = e.snapshot()
    assert sum(len(items) for _prio, items in snap.prefill.values()) > 0 and len(np.unique(snap.task_priority)) == 2
    got = t.tick(snap)
    want = o.tick(snap)
    print(f"two levels + a prefill set: {sum(len(r) for r in got.records)} records, {len(got.redirects)} redirects, {sum(len(r) for r in got.retracts)} retracts")
    _same(got, want)
    assert sum(len(r) for r in got.records) > 0
    t.close()


def test_one_placement_in_the_three_record_forms():
    from hyperqueue_amd.tick import Tick

    cfg = _cfg()
    snap = _env(cfg, [1, 2, 4, 3, 2], 48).snapshot()
    want = _oracle(cfg).tick(snap)
    for name, flags in (("plain", 0), ("compact", abi.HQTICK_FLAG_COMPACT_RECORDS), ("delta16", abi.HQTICK_FLAG_COMPACT_DELTA16)):
        t = Tick(_cfg(flags))
        got = t.tick(snap)
        print(f"{name}: {sum(len(r) for r in got.records)} records")
        _same(got, want)
        t.close()
    assert sum(len(r) for r in want.records) > 0


def test_empty_tick_publishes_a_well_formed_sink():
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import Tick

    cfg = _cfg()
    snap = _empty(_env(cfg, UNEQUAL, 8).snapshot())
    W = len(snap.worker_id)
    t = Tick(cfg)
    sink = _small_sink(W, 4)
    sink.fill_(0xAB)
    cap = t.set_record_sink(sink, W)
    rc = t.tick_raw(snap.to_c())
    assert rc.status == abi.HQTICK_DONE and not rc.rec_task
    assert [int(x) for x in np.ctypeslib.as_array(rc.rec_off, shape=(W + 1,))] == [0] * (W + 1)
    h = sink.cpu().numpy()
    n, _checksum, magic, hcap = [int(x) for x in h[:16].view(np.uint32)]
    o_off = sink_layout(W, cap)[0]
    print(f"empty tick: n {n}, magic {magic:#x}, capacity {hcap}")
    assert n == 0 and magic == SINK_MAGIC and hcap == cap == 4
    assert h[o_off:o_off + (W + 1) * 4].view(np.uint32).tolist() == [0] * (W + 1)
    t.set_record_sink(None)
    t.close()
