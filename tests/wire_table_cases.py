"""Delta sequences on the resident attribute table (hqwire_table_*, hyperqueue_amd.wire.WireTable) mirrored in a Python dict: shared by the CPU tests
(host debug backend), the GPU tests (device backend) and tools/wire_table_asan.py."""
import hashlib
import random

import numpy as np

import wire_cases as wc
from hyperqueue_amd import wire

TILE = wire.HQWIRE_TABLE_TILE
ENTRY_SIZES = [None, 0, 1, 15, 16, 17, 33, 4097]  # None, b"" (entry_some stays 1) and lengths around the 16-byte stores


def entry_of(rnd, size):
    return None if size is None else rnd.randbytes(size)


def rand_attr(rnd, n_cfg, big=False):
    size = rnd.choice(ENTRY_SIZES if big else ENTRY_SIZES[:-1] + [None, None, 5])
    return (rnd.randrange(50), rnd.randrange(1 << 32), rnd.randrange(1 << 64), rnd.randrange(n_cfg), entry_of(rnd, size))


def rand_configs(rnd, n):
    return [(None if rnd.random() < 0.5 else (rnd.randrange(10**6), rnd.randrange(10**9)), rnd.randbytes(rnd.choice([0, 1, 7, 64, 300]))) for _ in range(n)]


def digest(t: wire.WireTables) -> str:
    h = hashlib.sha256()
    for i, a in enumerate(t.arrays()):
        b = np.ascontiguousarray(a).tobytes()
        if i == 7:
            b = b[: int(t.entry_off[-1])]
        if i == 12:
            b = b[: int(t.body_off[-1])]
        h.update(len(b).to_bytes(8, "little") + b)
    return h.hexdigest()


def assert_equals_build(table: wire.WireTable, attrs, configs):
    """after a compaction: every array of the view is what WireTables.build makes from the live tasks (blobs compared up to their closing offset)"""
    got, want = table.copy_out(), wire.WireTables.build(attrs, configs)
    names = ["task_id", "task_rq", "task_instance", "task_priority", "task_config", "entry_some", "entry_off", "entry_blob", "config_time_some",
             "config_time_secs", "config_time_nanos", "body_off", "body_blob"]
    for name, g, w in zip(names, got.arrays(), want.arrays()):
        if name == "entry_blob":
            g, w = g[: int(got.entry_off[-1])], w[: int(want.entry_off[-1])]
        if name == "body_blob":
            g, w = g[: int(got.body_off[-1])], w[: int(want.body_off[-1])]
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name


def check_encode(rnd, encode, table, attrs, configs, n_workers=4, max_rec=40):
    """a random tick over LIVE tasks (prefill kinds, a retract list, a multi-node record) encoded on the table's view: the oracle's bytes for the dict"""
    live = sorted(attrs)
    pool = live[:]
    rnd.shuffle(pool)
    worker_ids = sorted(rnd.sample(range(1, 500), n_workers))
    records, retracts = [], []
    for w in range(n_workers):
        recs = []
        for _ in range(min(len(pool), rnd.randint(0, max_rec))):
            kind = rnd.choice([0, 1, 1])
            recs.append((pool.pop(), 0xFF if kind == 0 else rnd.randrange(4), kind))
        records.append(recs)
        retracts.append([rnd.randrange(1, 1 << 40) for _ in range(3)] if w == 1 else [])
    mn = [(pool.pop(), [2, 0, 3])] if pool else []
    r = wire.WireRecords.build(worker_ids, records, retracts, mn)
    res = encode(table, r, 1 << 22)
    assert res.status == wire.HQWIRE_OK and (res.slot_status == 0).all()
    assert res.messages(r) == wc.oracle_messages(attrs, configs, worker_ids, records, retracts, mn)


CFG = [(None, b"prog-a" * 9), ((60, 5), b"")]


def attrs_of(ids, entry=lambda i, t: None, cfg=0):
    return {t: (i % 7, i, (0x80000000 + i % 3) << 32, cfg, entry(i, t)) for i, t in enumerate(ids)}


def fresh(make_table, ids, entry=lambda i, t: None, **kw):
    """a table with the two configurations of CFG and one row per id"""
    t = make_table(**kw)
    t.add_configs(CFG)
    a = attrs_of(ids, entry)
    if a:
        assert t.add_tasks(a) == len(a)
    return t, a


def tile_boundary_case(make_table, encode, rows):
    """first and last row, rows across a tile boundary and a whole tile removed; after each an encode on the view with dead rows, then a compaction"""
    ids = [(2 << 32) | (10 + 3 * i) for i in range(rows)]
    ent = lambda i, t: None if i % 3 else bytes([i & 0xFF]) * (i % 40)
    t, a = fresh(make_table, ids, ent)
    rnd = random.Random(rows)
    for gone in ([ids[0], ids[-1]], ids[TILE - 3:TILE + 2] if rows > TILE else ids[5:9], ids[:TILE] if rows >= TILE else ids[20:60]):
        gone = [g for g in gone if g in a]
        assert t.remove_tasks(gone) == len(gone)
        for g in gone:
            del a[g]
        if a:
            check_encode(rnd, encode, t, a, CFG)
        t.compact()
        assert_equals_build(t, a, CFG)
        assert t.counters()["physical_rows"] == len(a)
    t.close()


def entry_sizes_case(make_table, encode):
    """None, b"" (entry_some stays 1), 1, 15, 16, 17, 33 and 4097 bytes on neighbouring rows, in rotating sequence so that sources and destinations fall on
    every alignment; through append, compaction (partly dead tiles and a full one), merge and growth"""
    sizes = ENTRY_SIZES
    rnd = random.Random(7)
    ids = [(3 << 32) | (2 * i + 2) for i in range(TILE + 40)]
    ent = lambda i, t: entry_of(rnd, sizes[(i + i // len(sizes)) % len(sizes)] if i < 40 or i >= TILE else [None, 3, 0][i % 3])
    t, a = fresh(make_table, ids, ent, initial_rows=16, initial_blob_bytes=32)
    assert t.copy_out().entry_some.tolist() == [0 if a[i][4] is None else 1 for i in sorted(a)]
    check_encode(rnd, encode, t, a, CFG, max_rec=80)
    for k in range(4):
        gone = [i for j, i in enumerate(sorted(a)) if j % 5 == k and j < 45]
        assert t.remove_tasks(gone) == len(gone)
        for g in gone:
            del a[g]
        t.compact()
        assert_equals_build(t, a, CFG)
        more = {g + 1: (1, 2, 3, 1, entry_of(rnd, sizes[(j + k) % len(sizes)])) for j, g in enumerate(gone[:8])}  # odd ids: between the old ones
        assert t.add_tasks(more) == len(more)
        a.update(more)
        assert_equals_build(t, a, CFG)
        check_encode(rnd, encode, t, a, CFG, max_rec=80)
    assert t.counters()["merges"] == 4
    t.close()


class Mirror:
    """the table as a dict, plus which removed ids still occupy a row"""

    def __init__(self):
        self.attrs, self.configs, self.dead, self.top = {}, [], set(), 0

    def add(self, batch):
        self.attrs.update(batch)
        self.dead -= set(batch)
        self.top = max(self.top, max(batch))


def run_sequence(seed, table: wire.WireTable, encode, n_ops=22, max_rows=3 * TILE, after_op=None):
    """Random deltas on `table`, mirrored; after every op an encode on the view against the oracle and the counts against the mirror; after every
    compaction copy_out against WireTables.build.  `after_op(table, mirror)` runs after every op (cross-backend comparisons)."""
    rnd = random.Random(seed)
    m = Mirror()
    m.configs += rand_configs(rnd, rnd.randint(1, 3))
    assert table.add_configs(m.configs) == 0
    job = rnd.randint(1, 3) << 32
    for op_i in range(n_ops):
        live = sorted(m.attrs)
        op = rnd.choice(["append", "append", "merge", "remove", "remove", "inc", "assign", "configs", "compact"]) if live else "append"
        before = table.counters()
        if op == "append":
            n = rnd.choice([1, 2, 7, TILE - 1, TILE + 1, rnd.randint(1, 300)])
            n = max(1, min(n, max_rows - len(live)))
            base = m.top + rnd.choice([1, 1, 5, 1 << 33])
            if m.top == 0:
                base = job + 1000
            ids = sorted(rnd.sample(range(base, base + 3 * n), n))
            batch = {t: rand_attr(rnd, len(m.configs), big=(op_i % 5 == 0 and k < 9)) for k, t in enumerate(ids)}
            assert table.add_tasks(batch) == n
            m.add(batch)
            assert table.counters()["appends"] == before["appends"] + 1
        elif op == "merge":
            n = max(1, min(rnd.choice([1, 3, 40]), max_rows - len(live)))
            cand = set(rnd.sample(sorted(m.dead), min(len(m.dead), n // 2 + 1)))          # ids equal to dead rows' ids
            cand |= {rnd.randrange(1, live[0]) for _ in range(n)}                           # below every resident id
            cand |= {rnd.randrange(live[0], max(live[-1], live[0] + 1)) for _ in range(n)}  # between
            ids = sorted(t for t in cand if t not in m.attrs and t > 0)[:n]
            if not ids or ids[0] >= live[-1]:
                continue
            batch = {t: rand_attr(rnd, len(m.configs), big=(op_i % 4 == 0)) for t in ids}
            assert table.add_tasks(batch) == len(ids)
            m.add(batch)
            m.dead.clear()  # a merge drops the dead rows first
            after = table.counters()
            assert after["merges"] == before["merges"] + 1 and after["physical_rows"] == len(m.attrs)
        elif op == "remove":
            k = rnd.choice([1, 2, len(live) // 3, len(live) // 2 + 1, len(live)]) if rnd.random() < 0.8 else len(live)
            gone = rnd.sample(live, max(1, min(k, len(live))))
            extra = [gone[0]] + [rnd.randrange(1, 1 << 50) for _ in range(2)] + list(m.dead)[:2]  # repeated, unknown (almost surely), already removed
            extra = [t for t in extra if t == gone[0] or t not in m.attrs]
            ids = gone + extra
            rnd.shuffle(ids)
            assert table.remove_tasks(ids) == len(gone)
            assert table.last_unknown() == len(extra)
            for t in gone:
                del m.attrs[t]
            m.dead |= set(gone)
            if table.counters()["compactions"] != before["compactions"]:
                m.dead.clear()
                assert_equals_build(table, m.attrs, m.configs)
        elif op == "inc":
            ids = rnd.sample(live, min(len(live), rnd.randint(1, 20)))
            ids.append(ids[0])  # listed twice: rises by two
            assert table.set_instance(ids) == len(ids)
            for t in ids:
                a = m.attrs[t]
                m.attrs[t] = (a[0], (a[1] + 1) & 0xFFFFFFFF, a[2], a[3], a[4])
        elif op == "assign":
            ids = rnd.sample(live, min(len(live), rnd.randint(1, 20)))
            vals = [rnd.randrange(1 << 32) for _ in ids]
            unknown = list(m.dead)[:1] + [rnd.randrange(1, 1 << 50) | (1 << 51)]
            assert table.set_instance(ids + unknown, vals + [7] * len(unknown)) == len(ids)
            assert table.last_unknown() == len(unknown)
            for t, v in zip(ids, vals):
                a = m.attrs[t]
                m.attrs[t] = (a[0], v, a[2], a[3], a[4])
        elif op == "configs":
            more = rand_configs(rnd, rnd.randint(1, 2))
            assert table.add_configs(more) == len(m.configs)
            m.configs += more
        elif op == "compact":
            table.compact()
            assert table.counters()["compactions"] == before["compactions"] + (1 if m.dead else 0)
            m.dead.clear()
            assert_equals_build(table, m.attrs, m.configs)
        st = table.counters()
        assert st["live_rows"] == len(m.attrs) and st["n_configs"] == len(m.configs)
        assert st["physical_rows"] >= st["live_rows"]
        if st["physical_rows"] == st["live_rows"]:
            m.dead.clear()  # (an add that ran out of room dropped them)
        assert st["physical_rows"] - st["live_rows"] == len(m.dead)
        if m.attrs:
            check_encode(rnd, encode, table, m.attrs, m.configs)
        if after_op:
            after_op(table, m)
    table.compact()
    assert_equals_build(table, m.attrs, m.configs)
    return m


def chained_ticks(table: wire.WireTable, driver, n_ticks=3):
    """Three ticks of a small cluster (6 workers, about 200 tasks in all) with ONE table fed by the reactor's events, a dict kept beside it.  Between
    ticks: new tasks enter the ready set and the table; the tasks placed in the tick before the last are finished -- released from the ledger, removed
    from the table --; one worker is lost and the ids the ledger reports as requeued go through set_instance (increment_instance_id).  `driver`:
      tick(snap, want) -> WireResult of the tick's messages, encoded on `table`      release(ids)      lose(wid, back) -> requeued ids
    Every tick's messages must be the bincode oracle's for the dict, and the requeued tasks must travel with their raised instance id."""
    import dataclasses

    from hyperqueue_amd import abi
    from hyperqueue_amd.core import SchedEnv, TaskBuilder as TB, WorkerBuilder as WB
    from oracle.oracle import Oracle

    rnd = random.Random(21)
    env = SchedEnv(abi.make_config(time_limit_s=20.0))
    env.new_workers(6, WB(16))
    configs = [(None, b"prog-a" * 30), ((600, 0), b"prog-b" * 70), ((5, 250), b"")]
    assert table.add_configs(configs) == 0
    attrs, bumped, placed_in = {}, {}, []
    shapes = [TB().cpus(0.25), TB().cpus(0.5).user_priority(1), TB().cpus(0.25).user_priority(2)]
    for k in range(n_ticks):
        new = []
        for n, shape in zip(([70, 30, 20], [30, 10, 10], [20, 10, 10])[k], shapes):
            new += env.new_tasks(n, shape)
        batch = {t: (env.tasks[t].rq, rnd.randrange(50), env.tasks[t].priority, rnd.randrange(3), None if rnd.random() < 0.6 else b"e-%d" % (t & 0xFFFF)) for t in new}
        assert table.add_tasks(batch) == len(batch) and table.counters()["merges"] == 0  # ids are minted ascending: appends
        attrs.update(batch)
        snap = dataclasses.replace(env.snapshot(), worker_map_rank=None, _keep=[])
        want = Oracle(env.config, canonical=True).tick(snap)
        worker_ids = [int(w) for w in snap.worker_id]
        res = driver.tick(snap, want)
        side = wire.WireRecords.build(worker_ids, want.records, want.retracts, [])
        assert res.status == wire.HQWIRE_OK and (res.slot_status == 0).all()
        msgs = res.messages(side)
        assert msgs == wc.oracle_messages(attrs, configs, worker_ids, want.records, want.retracts, [])
        sent = {d["id"]: d["instance_id"] for _, b in msgs for m in [wc.decode_message(b)] if m[0] == "compute" for d in m[1]}
        assert not any(want.retracts) and all(kind == 1 for recs in want.records for (_, _, kind) in recs)  # (room for everything: no prefill)
        assert set(sent) >= set(new) | set(bumped)
        for t, inst in bumped.items():  # requeued after the last tick: placed again, with the raised instance id
            assert sent[t] == inst == attrs[t][1]
        env.apply(want)
        placed_in.append(sorted(sent))
        if k + 1 == n_ticks:
            break
        if k >= 1:  # the tasks of the tick before this one finish
            done = [t for t in placed_in[k - 1] if env.tasks[t].state in (1, 2)]  # Assigned / Running
            for t in done:
                env.finish_task(t, env.tasks[t].worker)
                del attrs[t]
            driver.release(done)
            assert table.remove_tasks(done) == len(done) and table.last_unknown() == 0
        wid = max(env.workers, key=lambda w: (len(env.workers[w].assigned_tasks), w))
        back = sorted(env.workers[wid].assigned_tasks)
        assert back and env.remove_worker(wid) == []
        requeued = driver.lose(wid, back)
        assert sorted(requeued) == back
        assert table.set_instance(requeued) == len(back) and table.last_unknown() == 0
        bumped = {}
        for t in back:
            a = attrs[t]
            attrs[t] = (a[0], a[1] + 1, a[2], a[3], a[4])
            bumped[t] = a[1] + 1
    return attrs, configs
