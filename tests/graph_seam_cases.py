"""The seams of the device-resident dependency graph (csrc/graph.hip), as histories that cross each of them on purpose, and the one runner that plays a
history on the graph and on oracle/graph_oracle.py side by side.

Pure numpy + the graph oracle: nothing here imports the GPU side, so tests/test_graph_seam_cases.py can check on a machine without a GPU that every history
builds what it says it builds (run lengths, list sizes, hash buckets, pool sums).  tests/test_gpu_graph_seams.py plays the same histories on the MI355X.

A history is a list of steps:
    ("add", tasks)                 tasks = [(id, priority, request id, [dependency ids])], in submission order
    ("take", ids)                  the tick hands these ready tasks out (hqtick_ready_remove / GraphOracle.take_from_ready)
    ("finish", ids)
    ("finish_waiting", id)         hqtick_graph_finish of a task that still waits: refused with HQTICK_E_INVALID, and the task leaves the graph all the same
    ("remove", ids, recursive)
    ("blevel",)
    ("bad_add", tasks, code)       a batch the graph must refuse with `code`, leaving everything as it was
    ("stats", {field: expected})   fields of hqtick_graph_stats
    ("payload",)                   one resident tick against the oracle's tick on the oracle's ready set: the (priority, request) that travelled with every id
    ("drain",)                     take and finish everything ready, wave after wave, until the graph is empty: walks every edge list once
After every step the runner compares the whole observable state, for EVERY id the history ever named, with the oracle's."""
import re

import numpy as np

from hyperqueue_amd import abi
from oracle.graph_oracle import GraphOracle

# ---- the constants of csrc/graph.hip the histories are built around (test_graph_seam_cases.py reads them back from the source) ---------------------------
SHORT_RUN = 4                # runs up to this length are released by the thread that owns the finished task
RUN_CHUNK = 4096             # longer runs: chunks of this many edges, one wavefront each
SORT_CH = 4096               # elements one workgroup sorts in LDS; above it the network goes through global steps
BFS_LEVELS_PER_SYNC = 8      # levels of a recursive removal between two looks at the counters; a b-level group is this many sweeps + 1
MIN_HASH_CAP = 8192
MIN_SLOT_CAP = 4096
MIN_EDGE_CAP = 16384
SWEEPS_PER_GROUP = BFS_LEVELS_PER_SYNC + 1


def hash_rebuild_due(keys_and_tombstones: int, n: int, capacity: int) -> bool:
    return (keys_and_tombstones + n) * 2 > capacity


def compaction_due(edge_top: int, E: int, cap_edges: int) -> bool:
    return edge_top + E > cap_edges


MAX_ID = 0xFFFFFFFFFFFFFFFD  # include/hqtick.h: task ids >= 0xFFFFFFFFFFFFFFFE are reserved
GONE = 0xFFFFFFFF
_M64 = (1 << 64) - 1


def source_constants(text: str) -> dict:
    """the same constants, read from the text of csrc/graph.hip"""
    def one(pat):
        m = re.search(pat, text)
        assert m, f"csrc/graph.hip no longer matches {pat!r}: restate the constant in tests/graph_seam_cases.py and move the seams"
        return m.group(1) if m.groups() else True
    return {
        "SHORT_RUN": int(one(r"constexpr\s+uint32_t\s+SHORT_RUN\s*=\s*(\d+)\s*;")),
        "RUN_CHUNK": int(one(r"constexpr\s+uint32_t\s+RUN_CHUNK\s*=\s*(\d+)\s*;")),
        "SORT_CH": int(one(r"constexpr\s+uint32_t\s+SORT_CH\s*=\s*(\d+)\s*;")),
        "BFS_LEVELS_PER_SYNC": int(one(r"constexpr\s+uint32_t\s+BFS_LEVELS_PER_SYNC\s*=\s*(\d+)\s*;")),
        "MIN_HASH_CAP": int(one(r"pow2_at_least\(want_entries \* 2\),\s*(\d+)\)")),
        "MIN_SLOT_CAP": int(one(r"std::max<uint64_t>\(want \+ want / 2,\s*(\d+)\)")),
        "MIN_EDGE_CAP": int(one(r"\(live \+ extra\) \* 2,\s*(\d+)\}")),
        "rebuild_rule": one(r"if \(\(ht_used \+ n\) \* 2 > ht_cap\)"),
        "compaction_rule": one(r"if \(\(uint64_t\)edge_top \+ extra <= cap_edges\) return 0;"),
        "short_run_rule": one(r"if \(len > SHORT_RUN\)"),
        "blevel_group": one(r"for \(uint32_t l = 0; l < BFS_LEVELS_PER_SYNC; l\+\+\) \{ hipLaunchKernelGGL\(k_g_blevel_sweep"),
    }


def ht_hash(ids) -> np.ndarray:
    """ht_hash of csrc/graph.hip: the murmur3 finaliser, low 32 bits"""
    k = np.atleast_1d(np.asarray(ids, np.uint64)).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33); k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33); k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def colliding_ids(bucket: int, capacity: int = MIN_HASH_CAP, hi: int = 400_000) -> list:
    """the ids of 1..hi whose home bucket in a table of `capacity` buckets is `bucket`, ascending"""
    ids = np.arange(1, hi + 1, dtype=np.uint64)
    return ids[(ht_hash(ids) & np.uint32(capacity - 1)) == bucket].tolist()


# priority and request id are functions of the id that differ between neighbouring ids: the payload that follows a sorted key is then checkable
def prio_of(i: int) -> int:
    return ((i * 2654435761) % 5) << 32


def rq_of(i: int) -> int:
    return (i // 7) % 3


def task(i: int, deps=()):
    return (i, prio_of(i), rq_of(i), list(deps))


def jobbed(n: int, base: int, ends: bool = False) -> list:
    """n ids with job bits 1..3 << 32 mixed in; ends: the smallest and the largest id include/hqtick.h allows are among them"""
    ids = [((k % 3 + 1) << 32) | (base + k) for k in range(n)]
    if ends:
        ids[0] = MAX_ID
        if n >= 2:
            ids[1] = 0
    return ids


def _pow2_at_least(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


# ================================================================================================================ the model
class PoolModel:
    """The host-side bookkeeping of Graph (graph.hip's host driver) in plain integers: slots, hash table and edge pool sizes as the rules above give them.
    What hqtick_graph_stats must report after every step of a history — known without a GPU."""

    def __init__(self):
        self.cap_slots = self.n_slots = self.free_top = 0
        self.ht_cap = self.ht_used = self.n_live = 0
        self.cap_edges = self.edge_top = self.run_top = self.edges_dead = 0
        self.chain = {}            # live task -> its run lengths, newest first
        self.compactions = 0
        self.hash_rebuilds = []    # (capacity before, capacity after)
        self.slot_growths = 0
        self.tombstones_exact = True

    def _capacity(self, n: int, E: int):
        fresh = max(0, n - self.free_top)
        if self.n_slots + fresh > self.cap_slots:
            want = self.n_slots + fresh
            self.cap_slots = max(want + want // 2, MIN_SLOT_CAP)
            self.slot_growths += 1
        if hash_rebuild_due(self.ht_used, n, self.ht_cap):
            nc = max(_pow2_at_least((self.n_live + n) * 2), MIN_HASH_CAP)
            nc = max(nc, self.ht_cap)  # not larger: rebuilt in place, which purges the tombstones
            self.hash_rebuilds.append((self.ht_cap, nc))
            self.ht_cap, self.ht_used, self.tombstones_exact = nc, self.n_live, True
        if compaction_due(self.edge_top, E, self.cap_edges):
            live = self.edge_top - self.edges_dead
            nc = max(self.cap_edges, (live + E) * 2, MIN_EDGE_CAP)
            if self.edge_top:  # every live producer's runs become one run (stale edges travel along)
                self.compactions += 1
                self.chain = {p: [sum(r)] for p, r in self.chain.items() if r}
                self.run_top = len(self.chain)
                self.edge_top, self.edges_dead = sum(r[0] for r in self.chain.values()), 0
            self.cap_edges = nc
        return fresh

    def add(self, tasks, g: GraphOracle) -> dict:
        """before g.on_new_tasks(tasks).  Returns {producer: length of the run this batch gives it}"""
        n, E = len(tasks), sum(len(t[3]) for t in tasks)
        info = {"edge_top_before": self.edge_top, "E": E, "cap_edges_before": self.cap_edges, "compactions_before": self.compactions,
                "ht_used_before": self.ht_used, "ht_cap_before": self.ht_cap, "free_top_before": self.free_top, "n_slots_before": self.n_slots}
        fresh = self._capacity(n, E)
        present, runs = set(g.tasks), {}
        for i, _, _, deps in tasks:  # reactor.rs:193-203: a dependency is kept only if the task map holds it when the consumer is processed
            for d in deps:
                if d in present:
                    runs[d] = runs.get(d, 0) + 1
            present.add(i)
        for p, ln in runs.items():
            self.chain.setdefault(p, []).insert(0, ln)
        self.run_top += len(runs); self.edge_top += sum(runs.values())
        assert self.edge_top <= self.cap_edges
        self.free_top -= min(n, self.free_top); self.n_slots += fresh; self.n_live += n; self.ht_used += n
        info.update(runs=runs, compacted=self.compactions != info["compactions_before"])
        return info

    def refused(self, tasks):
        ids = [t[0] for t in tasks]
        if any(i > MAX_ID for i in ids):
            return  # refused on the host before anything is sized
        self._capacity(len(tasks), sum(len(t[3]) for t in tasks))
        if len(set(ids)) != len(ids):  # the rolled-back batch's keys count as tombstones, whether or not they were inserted: an upper estimate from here on
            self.ht_used += len(ids); self.tombstones_exact = False

    def gone(self, ids):
        """finished or removed tasks: slots to the free stack, keys to tombstones, their runs dead"""
        for i in ids:
            self.edges_dead += sum(self.chain.pop(i, []))
        self.free_top += len(ids); self.n_live -= len(ids)

    def stats(self) -> dict:
        return {"n_tasks": self.n_live, "n_slots": self.n_slots, "n_edges_live": self.edge_top - self.edges_dead, "n_edges_pool": self.edge_top, "n_runs": self.run_top,
                "hash_capacity": self.ht_cap, "hash_tombstones": self.ht_used - self.n_live}


# ================================================================================================================ the runner
def _add(T, tasks):
    return T.graph_add_tasks([t[0] for t in tasks], [t[1] for t in tasks], [t[2] for t in tasks], [list(t[3]) for t in tasks]).tolist()


def _last_unknown(T) -> int:
    import ctypes as C
    f = T._lib.hqtick_graph_last_unknown
    f.restype, f.argtypes = C.c_uint64, [C.c_void_p]
    return int(f(T._ctx))


def _ascending(ids):
    assert all(a < b for a, b in zip(ids, ids[1:])), "the id list is not strictly ascending"


def _check_state(T, g, minted, where):
    if T is None:
        return
    assert T.ready_count() == len(g.ready), where
    assert T.graph_stats()["n_tasks"] == len(g.tasks), where
    got = T.graph_unfinished(np.asarray(minted, np.uint64))
    want = np.asarray([g.unfinished(i) for i in minted], np.uint32)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{where}: unfinished of id {minted[int(bad[0])]:#x} is {int(got[bad[0]]):#x}, the oracle says {int(want[bad[0]]):#x} ({len(bad)} ids differ)"


def _payload(T, g):
    """the recipe of test_gpu_graph.py::test_ready_set_after_graph_ops_ticks_like_the_oracle: three request ids on one request, so the oracle's solve is trivial;
    `counts` carries the request id and `records` the ids in priority order, so a (priority, request) that went with the wrong id shows"""
    from hyperqueue_amd import workloads
    from oracle.oracle import Oracle

    base = workloads.make("c1")
    ids = np.asarray(sorted(g.ready), np.uint64)
    assert len(ids) > 0
    snap_kw = {f: getattr(base, f) for f in ("n_resources", "worker_id", "worker_total", "worker_free", "worker_remaining_ns", "worker_min_utilization", "worker_flags",
                                             "worker_group", "n_groups", "blocked", "assigned", "prefilled", "prefill", "worker_map_rank")}
    reqs = [base.requests[0]] * 3
    full = abi.Snapshot(**snap_kw, requests=reqs, task_id=ids, task_priority=np.asarray([g.ready[int(i)][0] for i in ids], np.uint64),
                        task_rq=np.asarray([g.ready[int(i)][1] for i in ids], np.uint32))
    stripped = abi.Snapshot(**snap_kw, requests=reqs, task_id=np.zeros(0, np.uint64), task_priority=np.zeros(0, np.uint64), task_rq=np.zeros(0, np.uint32))
    want = Oracle(abi.make_config(time_limit_s=20.0), canonical=True).tick(full)
    assert sum(len(r) for r in want.records) > 0
    if T is None:
        return
    got = T.tick(stripped, resident=True)
    assert got.batches == want.batches and got.counts == want.counts and got.records == want.records


def run(T, steps):
    """Plays `steps` on the Tick `T` and on a GraphOracle, comparing after every step.  T = None: the oracle and the model alone (no GPU), which still checks every
    "stats" step against PoolModel.  Returns (oracle, model, log); log has one dict per step with what the step produced."""
    g, m, log = GraphOracle(), PoolModel(), []
    minted, seen, running = [], set(), set()

    def mint(ids):
        for i in ids:
            if i not in seen and i <= MAX_ID:
                seen.add(i); minted.append(i)

    def finish(ids, where):
        known = [i for i in dict.fromkeys(ids) if i in g.tasks]
        want, unk_w = g.task_finished(ids)
        m.gone(known)
        running.difference_update(ids)
        if T is not None:
            rel, unk = T.graph_finish(ids)
            _ascending(rel.tolist())
            assert rel.tolist() == want and unk == unk_w, where
        return want, unk_w

    for k, st in enumerate(steps):
        op, where, entry = st[0], f"step {k} ({st[0]})", {"op": st[0]}
        if op == "add":
            tasks = st[1]
            mint(t[0] for t in tasks); mint(d for t in tasks for d in t[3])
            entry.update(m.add(tasks, g))
            want = g.on_new_tasks(tasks)
            entry["n_out"] = len(want)
            if T is not None:
                got = _add(T, tasks)
                _ascending(got)
                assert got == want, where
        elif op == "bad_add":
            tasks, code = st[1], st[2]
            mint(t[0] for t in tasks)
            m.refused(tasks)
            if T is not None:
                try:
                    _add(T, tasks)
                except Exception as e:  # hyperqueue_amd.tick.HqTickError
                    assert getattr(e, "code", None) == code, where
                else:
                    raise AssertionError(f"{where}: the batch was accepted")
        elif op == "take":
            ids = list(st[1])
            g.take_from_ready(ids)
            running.update(ids)
            if T is not None:
                assert T.ready_remove(np.asarray(ids, np.uint64)) == len(ids), where
        elif op == "finish":
            ids = list(st[1])
            mint(ids)
            want, unk = finish(ids, where)
            entry.update(n_out=len(want), unknown=unk)
        elif op == "finish_waiting":
            # EXISTING BEHAVIOUR, pinned as it is: hqtick_graph_finish of a task that still has unfinished dependencies reports HQTICK_E_INVALID (the reference hits
            # unreachable!(), reactor.rs:551-555) and removes the task all the same.  For a task nothing depends on, that is the oracle's non-recursive removal.
            i = st[1]
            assert g.tasks[i].unfinished > 0 and not g.tasks[i].consumers
            g.remove([i], False)
            m.gone([i])
            if T is not None:
                try:
                    T.graph_finish([i])
                except Exception as e:
                    assert getattr(e, "code", None) == abi.HQTICK_E_INVALID, where
                else:
                    raise AssertionError(f"{where}: finishing a waiting task was not reported")
                assert T.graph_unfinished([i]).tolist() == [GONE], where
        elif op == "remove":
            ids, rec = list(st[1]), bool(st[2])
            mint(ids)
            want, unk_w = g.remove(ids, rec)
            m.gone(want)
            running.difference_update(want)
            entry.update(n_out=len(want), unknown=unk_w)
            if T is not None:
                got = T.graph_remove(np.asarray(ids, np.uint64), recursive=rec).tolist()
                _ascending(got)
                assert got == want and _last_unknown(T) == unk_w, where
        elif op == "blevel":
            depth = g.apply_blevels()
            entry["depth"] = depth
            if T is not None:
                info = T.graph_blevel(update_ready=True)
                live = sorted(g.tasks)
                assert info["max_level"] == depth and info["ready_updated"] == len(g.ready), where
                assert info["sweeps"] >= 1 and info["sweeps"] % SWEEPS_PER_GROUP == 0, where
                if live:
                    assert T.graph_priorities(np.asarray(live, np.uint64)).tolist() == [g.tasks[i].priority for i in live], where
        elif op == "stats":
            have = m.stats()
            for f, v in st[1].items():
                assert f != "hash_tombstones" or m.tombstones_exact, "after a rolled-back batch hash_tombstones is an upper estimate: do not state it"
                assert have[f] == v, f"{where}: the history states {f} = {v}, the rules give {have[f]}"
            if T is not None:
                got = T.graph_stats()
                for f, v in st[1].items():
                    assert got[f] == v, f"{where}: {f} is {got[f]}, expected {v}"
        elif op == "payload":
            _payload(T, g)
        elif op == "drain":
            waves = 0
            while g.tasks:
                ready = sorted(g.ready)
                if ready:
                    g.take_from_ready(ready)
                    running.update(ready)
                    if T is not None:
                        assert T.ready_remove(np.asarray(ready, np.uint64)) == len(ready), where
                batch = sorted(running)
                assert batch, f"{where}: tasks are left that nothing can release"
                finish(batch, f"{where}, wave {waves}")
                waves += 1
                _check_state(T, g, minted, f"{where}, wave {waves}")
            entry["waves"] = waves
        else:
            raise ValueError(op)
        _check_state(T, g, minted, where)
        log.append(entry)
    return g, m, log


# ================================================================================================================ the histories
# ---- A. run lengths -----------------------------------------------------------------------------------------------------------------------------------------
RUN_COUNTS = (1, SHORT_RUN, SHORT_RUN + 1, 63, 64, 65, RUN_CHUNK - 1, RUN_CHUNK, RUN_CHUNK + 1, 2 * RUN_CHUNK, 2 * RUN_CHUNK + 1)   # 28 875 consumers


def case_run_lengths(order: str):
    """eleven producers whose single runs sit on every side of SHORT_RUN and RUN_CHUNK, and a gate every consumer also waits for: one run of 28 875, eight chunks,
    the last of 203.  order "producers_first": nothing is released until the gate goes; "gate_first": the eleven release everything in one call"""
    prods, gate = list(range(1, 12)), 12
    cons, k = [], 0
    for p, c in zip(prods, RUN_COUNTS):
        for _ in range(c):
            cons.append(task(((k % 3 + 1) << 32) | (100 + k), [p, gate])); k += 1
    cons = [cons[j] for j in np.random.default_rng(1).permutation(len(cons))]
    steps = [("add", [task(i) for i in prods + [gate]]), ("add", cons), ("take", prods + [gate])]
    steps += [("finish", prods), ("finish", [gate])] if order == "producers_first" else [("finish", [gate]), ("finish", prods)]
    return steps + [("payload",)]


# ---- B. a chain that mixes short and long runs, with stale edges in the long one -------------------------------------------------------------------------------
MIXED_RUNS = (3, RUN_CHUNK + 1, 5)


def case_mixed_chain():
    p1, p2 = 1, 2
    a, b, c = jobbed(MIXED_RUNS[0], 10), jobbed(MIXED_RUNS[1], 1000), jobbed(MIXED_RUNS[2], 6000)
    victims = b[::7]                                  # leave the graph before p1 finishes: their edges in the long run go stale
    heirs = jobbed(len(victims), 10_000)              # as many new tasks: they move into the freed slots, and wait for p2, not p1
    return [("add", [task(p1), task(p2)]), ("add", [task(i, [p1]) for i in a]), ("add", [task(i, [p1]) for i in b]), ("add", [task(i, [p1]) for i in c]),
            ("remove", victims, False), ("add", [task(i, [p2]) for i in heirs]),
            ("take", [p1]), ("finish", [p1]),         # releases exactly the survivors; every heir still has unfinished == 1
            ("blevel",), ("drain",)]


# ---- C. sort sizes ------------------------------------------------------------------------------------------------------------------------------------------
SORT_SIZES = (1, 2, 3, SORT_CH - 1, SORT_CH, SORT_CH + 1, 2 * SORT_CH - 1, 2 * SORT_CH, 2 * SORT_CH + 1, 3 * SORT_CH + 1)
SORT_SIZES_SHORT = (3, SORT_CH, SORT_CH + 1, 2 * SORT_CH + 1)   # the short-path finish and the recursive removal need only these
SORT_SIZES_PAYLOAD = (SORT_CH + 1, 2 * SORT_CH + 1)


def case_sort_size(n: int):
    """every output list of the graph at exactly n entries (n + 1 for the removal): the ready-now list of an add submitted in descending id order, the released list
    of n one-consumer producers (short path), of one hub with n consumers (wide path), the removed list of a hub with n consumers"""
    roots = jobbed(n, 1, ends=True)
    steps = [("add", [task(i) for i in sorted(roots, reverse=True)])]                 # ready-now: n
    if n in SORT_SIZES_SHORT:
        steps.append(("add", [task(c, [r]) for c, r in zip(jobbed(n, 100_000), roots)]))
    shuffled = [roots[j] for j in np.random.default_rng(n).permutation(n)]
    steps += [("take", roots), ("finish", shuffled)]                                  # released: n (short path) or nothing; ids 0 and MAX_ID are free again
    if n in SORT_SIZES_SHORT:
        hub2 = 7
        steps += [("add", [task(hub2)]), ("add", [task(i, [hub2]) for i in jobbed(n, 300_000)]), ("remove", [hub2], True)]   # removed: n + 1
    hub = 5
    steps += [("add", [task(hub)]), ("add", [task(i, [hub]) for i in jobbed(n, 200_000, ends=True)]), ("take", [hub]), ("finish", [hub])]   # released: n
    steps += [("bad_add", [task(9), task(0xFFFFFFFFFFFFFFFE)], abi.HQTICK_E_INVALID), ("bad_add", [task(0xFFFFFFFFFFFFFFFF), task(9)], abi.HQTICK_E_INVALID)]
    if n in SORT_SIZES_PAYLOAD:
        steps.append(("payload",))
    return steps


# ---- D. depth of the recursive removal ----------------------------------------------------------------------------------------------------------------------
BFS_CHAINS = (1, BFS_LEVELS_PER_SYNC - 1, BFS_LEVELS_PER_SYNC, BFS_LEVELS_PER_SYNC + 1, BFS_LEVELS_PER_SYNC + 2, 2 * BFS_LEVELS_PER_SYNC, 2 * BFS_LEVELS_PER_SYNC + 1,
              2 * BFS_LEVELS_PER_SYNC + 2)


def case_bfs_chain(n: int):
    """a chain of n tasks removed from its head; beside it a chain that stays, and a producer whose only consumer hangs on the middle of the removed chain"""
    chain = list(range(1, n + 1))
    stay = [101, 102, 103]
    tasks = [task(chain[0])] + [task(chain[k], [chain[k - 1]]) for k in range(1, n)]
    tasks += [task(stay[0])] + [task(stay[k], [stay[k - 1]]) for k in (1, 2)] + [task(200), task(201, [200, chain[n // 2]])]
    return [("add", tasks), ("remove", [chain[0]], True), ("drain",)]


def case_bfs_diamond():
    """depth 9; task 6 is reachable over 1-2-3-6 and, on the same level from two sides, over 1-4-6 and 1-5-6: removed once"""
    tasks = [task(1), task(2, [1]), task(3, [2]), task(4, [1]), task(5, [1]), task(6, [3, 4, 5])] + [task(k, [k - 1]) for k in range(7, 13)] + [task(50), task(51, [50])]
    return [("add", tasks), ("blevel",), ("remove", [1], True), ("drain",)]


def case_bfs_victims():
    """a victim list naming a task, one of its descendants, the first again and an unknown id: removed once each, unknown == 1"""
    tasks = [task(1)] + [task(k, [k - 1]) for k in range(2, 6)]
    return [("add", tasks), ("remove", [2, 4, 2, 999], True), ("drain",)]


# ---- E. depth of the b-level sweeps ---------------------------------------------------------------------------------------------------------------------------
BLEVEL_DEPTHS = (0, 1, BFS_LEVELS_PER_SYNC, SWEEPS_PER_GROUP, SWEEPS_PER_GROUP + 1, 2 * SWEEPS_PER_GROUP - 1, 2 * SWEEPS_PER_GROUP, 3 * SWEEPS_PER_GROUP)
BLEVEL_SIDE = dict(zip(BLEVEL_DEPTHS, range(len(BLEVEL_DEPTHS))))   # a side branch of another length for each, never longer than the way to where it joins


def blevel_shape(d: int):
    main, side = list(range(1, d + 2)), list(range(101, 101 + BLEVEL_SIDE[d]))
    join = min(d, max(len(side), d // 2))
    return main, side, join


def case_blevel_depth(d: int):
    """a chain of depth d (d + 1 tasks) with a side branch joining in the middle; b-levels on the full graph, and again after the head is finished and a middle
    task removed with everything behind it"""
    main, side, join = blevel_shape(d)
    tasks = [task(s, [side[k - 1]] if k else []) for k, s in enumerate(side)]
    for k, t in enumerate(main):
        deps = [main[k - 1]] if k else []
        if k == join and side:
            deps.append(side[-1])
        tasks.append(task(t, deps))
    steps = [("add", tasks), ("blevel",), ("take", [main[0]]), ("finish", [main[0]])]
    if d >= 1:
        steps.append(("remove", [main[max(1, d // 2)]], True))
    return steps + [("blevel",), ("drain",)]


# ---- F. hash collisions -------------------------------------------------------------------------------------------------------------------------------------
CLUSTER = 24


def case_hash_cluster(bucket: int):
    """24 ids with one home bucket in a fresh 8192-bucket table (from bucket 8191 the cluster wraps to bucket 0); the 3rd to 10th leave, the ones behind them must
    still be found past the tombstones; two of the gone ids come back; a batch naming a live id of the cluster is refused"""
    c = colliding_ids(bucket)[:CLUSTER + 1]
    tasks = [task(c[k], [c[k - 12]] if 12 <= k < 18 else []) for k in range(CLUSTER)]
    return [("add", tasks), ("stats", {"hash_capacity": MIN_HASH_CAP, "hash_tombstones": 0}),
            ("take", c[2:6]), ("finish", c[2:6]), ("remove", c[6:10], False), ("stats", {"hash_tombstones": 8}),
            ("add", [task(c[3], [c[0]]), task(c[7], [c[1]])]),
            ("bad_add", [task(c[CLUSTER]), task(c[20])], abi.HQTICK_E_INVALID),
            ("add", [task(c[CLUSTER], [c[3], c[23]])]),
            ("stats", {"hash_capacity": MIN_HASH_CAP, "hash_tombstones": 8, "n_tasks": CLUSTER - 8 + 3}),
            ("drain",)]


# ---- G. hash rebuild ------------------------------------------------------------------------------------------------------------------------------------------
def case_hash_rebuild(n_more: int):
    """4000 tombstones in an 8192-bucket table: 95 more keys stay under the rebuild rule ((4000 + 95) * 2 = 8190), 97 cross it ((4000 + 97) * 2 = 8194) and the
    table is rebuilt in place; 5000 live tasks later it is rebuilt into 16384 buckets"""
    first = list(range(1, 4001))
    more = list(range(5001, 5001 + n_more))
    steps = [("add", [task(i) for i in first]), ("take", first), ("finish", first), ("stats", {"hash_tombstones": 4000, "hash_capacity": 8192, "n_tasks": 0}),
             ("add", [task(i, [i - 1] if i % 2 == 0 else []) for i in more])]
    if n_more == 95:
        steps += [("stats", {"hash_tombstones": 4000, "hash_capacity": 8192, "n_tasks": 95}),          # no rebuild
                  ("add", [task(5096, [5001]), task(5097, [5096, 3])])]                                  # (4095 + 2) * 2 = 8194: now, with 95 live keys to re-insert
    steps += [("stats", {"hash_tombstones": 0, "hash_capacity": 8192, "n_tasks": 97}),
              ("add", [task(10_000 + k, [5001 + k % 97]) for k in range(5000)]),
              ("stats", {"hash_tombstones": 0, "hash_capacity": 16384, "n_tasks": 5097}), ("drain",)]
    return steps


# ---- H. edge pool -------------------------------------------------------------------------------------------------------------------------------------------
def case_edge_pool(fit: str):
    """64 producers with 125 consumers each fill 8000 of 16384 edge slots; 32 producers finish (4000 dead edges).  "exact": the next batch brings edge_top + E to
    16384 and the pool is left alone; "over": one edge more, and the live runs are compacted into the other pool, one run per producer.  A later batch overflows
    the pool again: compacted back into the first pair of buffers."""
    prods = list(range(1, 65))
    E1 = MIN_EDGE_CAP - 8000 + (0 if fit == "exact" else 1)     # 8384 / 8385 edges on producers 33..48
    E2 = 12_386                                                 # on producers 49..64
    steps = [("add", [task(p) for p in prods]), ("add", [task(1000 + k, [1 + k % 64]) for k in range(8000)]),
             ("stats", {"n_edges_pool": 8000, "n_runs": 64, "n_edges_live": 8000}),
             ("take", prods[:32]), ("finish", prods[:32]),
             ("stats", {"n_edges_pool": 8000, "n_runs": 64, "n_edges_live": 4000}),
             ("add", [task(20_000 + k, [33 + k % 16]) for k in range(E1)])]
    if fit == "exact":   # 8000 + 8384 = 16384: no compaction, the 64 old runs stay and the batch's 16 producers get one each
        steps.append(("stats", {"n_edges_pool": 16384, "n_runs": 64 + 16, "n_edges_live": 16384 - 4000}))
    else:                # 8000 + 8385 = 16385: the 32 live producers keep one run of 125 each, then the batch's 16 runs
        steps.append(("stats", {"n_edges_pool": 32 * 125 + 8385, "n_runs": 32 + 16, "n_edges_live": 32 * 125 + 8385}))
    # producers 33..40 finish; 41..48 hold 125 + 524 edges each (E1 = 16 * 524 + 0 or 1, the odd one on 33), 49..64 hold 125
    steps += [("take", prods[32:40]), ("finish", prods[32:40]),
              ("add", [task(40_000 + k, [49 + k % 16]) for k in range(E2)]),
              ("stats", {"n_edges_pool": 8 * (125 + 524) + 16 * 125 + E2, "n_runs": 24 + 16, "n_edges_live": 8 * (125 + 524) + 16 * 125 + E2}),
              ("blevel",), ("drain",)]
    return steps


# ---- I. slots, J. rollback ----------------------------------------------------------------------------------------------------------------------------------
def _slot_state():
    """4096 tasks in 4096 slots, 100 of them finished: the free stack holds 100"""
    tasks = [task(i) for i in range(1, 2049)] + [task(i, [i - 2048]) for i in range(2049, 4097)]
    gone = list(range(1, 101))
    return [("add", tasks), ("take", gone), ("finish", gone), ("stats", {"n_slots": MIN_SLOT_CAP, "n_tasks": 3996})]


def case_slots(n: int):
    """a batch of 99, 100 or 101 on a free stack of 100: all from the stack, the stack exactly, the stack and one fresh slot.  Then 2100 more: the slot arrays grow
    past their first capacity (6144) and keep their contents"""
    batch = [task(10_000 + k, [101 + k, 2200 + k]) for k in range(n)]
    more = [task(20_000 + k, [10_000 + k % n]) for k in range(2100)]
    n_slots = MIN_SLOT_CAP + max(0, n - 100)
    return _slot_state() + [("add", batch), ("stats", {"n_slots": n_slots, "n_tasks": 3996 + n}),
                            ("add", more), ("stats", {"n_slots": n_slots + 2100 - max(0, 100 - n), "n_tasks": 3996 + n + 2100}), ("blevel",), ("drain",)]


def case_rollback():
    """a 600-task batch (three workgroups) that takes the 100 recycled slots and 500 fresh ones, names live producers, and carries its first id again at the end:
    refused, nothing changes; the same batch without the duplicate is accepted, and finishing its producers releases what the oracle releases"""
    ids = [30_000 + k for k in range(600)]
    good = [task(i, [101 + k, 2200 + k]) for k, i in enumerate(ids)]
    bad = good[:-1] + [(ids[0],) + good[-1][1:]]
    prods = list(range(101, 701))
    return _slot_state() + [("bad_add", bad, abi.HQTICK_E_INVALID), ("stats", {"n_slots": MIN_SLOT_CAP, "n_tasks": 3996}),
                            ("add", good), ("stats", {"n_slots": MIN_SLOT_CAP + 500, "n_tasks": 4596}),
                            ("take", prods), ("finish", prods),
                            ("finish_waiting", ids[-1]),   # 30 599 waits for 2799, which waits for 751
                            ("blevel",), ("drain",)]


CASES = {
    "run_lengths": (case_run_lengths, ("producers_first", "gate_first")),
    "mixed_chain": (case_mixed_chain, ((),)),
    "sort_size": (case_sort_size, SORT_SIZES),
    "bfs_chain": (case_bfs_chain, BFS_CHAINS),
    "bfs_diamond": (case_bfs_diamond, ((),)),
    "bfs_victims": (case_bfs_victims, ((),)),
    "blevel_depth": (case_blevel_depth, BLEVEL_DEPTHS),
    "hash_cluster": (case_hash_cluster, (MIN_HASH_CAP - 1, 0)),
    "hash_rebuild": (case_hash_rebuild, (95, 97)),
    "edge_pool": (case_edge_pool, ("exact", "over")),
    "slots": (case_slots, (99, 100, 101)),
    "rollback": (case_rollback, ((),)),
}


def build(family: str, arg=()):
    fn = CASES[family][0]
    return fn() if arg == () else fn(arg)
