"""tests/graph_seam_cases.py on its own, without a GPU: every history builds what it says it builds (on the graph oracle and the host-side model of the pools),
the constants it is built around are the ones csrc/graph.hip has, and the restated hash is the one the table uses."""
import functools
import os

import pytest

import graph_seam_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(f, a) for f, (_, args) in S.CASES.items() for a in args]


@functools.lru_cache(maxsize=None)
def _played(family, arg=()):
    """(oracle, model, log) of a history played on the oracle and the pool model alone; played once, shared by the tests that read it"""
    return S.run(None, S.build(family, arg))


def _adds(log):
    return [e for e in log if e["op"] == "add"]


def test_constants_are_those_of_the_source():
    """whoever changes one of them in csrc/graph.hip: restate it in graph_seam_cases.py, which moves the seams with it"""
    with open(os.path.join(ROOT, "hyperqueue_amd", "csrc", "graph.hip")) as f:
        src = S.source_constants(f.read())
    for name in ("SHORT_RUN", "RUN_CHUNK", "SORT_CH", "BFS_LEVELS_PER_SYNC", "MIN_HASH_CAP", "MIN_SLOT_CAP", "MIN_EDGE_CAP"):
        assert src[name] == getattr(S, name), name
    assert (S.SHORT_RUN, S.RUN_CHUNK, S.SORT_CH, S.BFS_LEVELS_PER_SYNC, S.MIN_HASH_CAP, S.MIN_SLOT_CAP, S.MIN_EDGE_CAP) == (4, 4096, 4096, 8, 8192, 4096, 16384)
    assert src["rebuild_rule"] and src["compaction_rule"] and src["short_run_rule"] and src["blevel_group"]
    # the rules as the histories use them
    assert not S.hash_rebuild_due(4000, 95, 8192) and (4000 + 95) * 2 == 8190
    assert S.hash_rebuild_due(4000, 97, 8192) and (4000 + 97) * 2 == 8194
    assert not S.compaction_due(8000, 8384, 16384) and S.compaction_due(8000, 8385, 16384)


def test_hash_restatement():
    assert S.ht_hash([0, 1]).tolist() == [0, 0x34C2CB2C]
    # the finaliser in plain Python integers
    def ref(k):
        M = (1 << 64) - 1
        k ^= k >> 33; k = (k * 0xFF51AFD7ED558CCD) & M; k ^= k >> 33; k = (k * 0xC4CEB9FE1A85EC53) & M; k ^= k >> 33
        return k & 0xFFFFFFFF
    ids = [2, 3, 12345, 1 << 32, (3 << 32) | 77, S.MAX_ID]
    assert S.ht_hash(ids).tolist() == [ref(i) for i in ids]
    assert len(S.colliding_ids(8191)) == 44 and len(S.colliding_ids(0)) == 58


@pytest.mark.parametrize("family,arg", ALL, ids=[f"{f}-{a}" if a != () else f for f, a in ALL])
def test_every_history_runs_on_the_oracle_and_its_stated_stats_follow_from_the_rules(family, arg):
    """run(None, ...) plays the history on the oracle and the pool model alone: every "stats" step is checked against the model, every take / finish against the
    oracle's own assertions (a task is finished only when it is ready and was handed out)"""
    g, m, log = _played(family, arg)
    steps = S.build(family, arg)
    assert len(log) == len(steps)
    if steps[-1][0] == "drain":
        assert not g.tasks and not g.ready


@pytest.mark.parametrize("order", S.CASES["run_lengths"][1])
def test_run_lengths_are_what_the_case_says(order):
    g, m, log = _played("run_lengths", order)
    adds = _adds(log)
    total = sum(S.RUN_COUNTS)
    assert total == 28_875 and sorted(adds[1]["runs"].values()) == sorted(S.RUN_COUNTS + (total,))
    assert {c for c in S.RUN_COUNTS} >= {4, 5, 4096, 4097}
    assert -(-total // S.RUN_CHUNK) == 8 and total - 7 * S.RUN_CHUNK == 203          # the gate's run: eight chunks, the last of 203
    assert m.n_slots == 28_887 and adds[1]["E"] == 57_750
    fin = [e for e in log if e["op"] == "finish"]
    assert [e["n_out"] for e in fin] == [0, total]                                    # whichever goes first releases nothing, the second everything


def test_mixed_chain_is_what_the_case_says():
    steps = S.case_mixed_chain()
    g, m, log = S.run(None, steps[:6])   # up to the heirs' batch: producer 1's chain, newest run first
    assert m.chain[1] == [5, S.RUN_CHUNK + 1, 3]
    victims = steps[4][1]
    assert len(victims) == 586 and m.free_top == 0 and _adds(log)[-1]["free_top_before"] == 586    # the heirs took exactly the freed slots
    g, m, log = _played("mixed_chain")
    fin = [e for e in log if e["op"] == "finish"][0]
    assert fin["n_out"] == 3 + 5 + 4097 - 586


@pytest.mark.parametrize("n", S.SORT_SIZES)
def test_sort_sizes_are_what_the_case_says(n):
    steps = S.case_sort_size(n)
    g, m, log = _played("sort_size", n)
    sizes = [e["n_out"] for e in log if "n_out" in e]
    assert sizes.count(n) >= (3 if n in S.SORT_SIZES_SHORT else 2)                    # ready-now, (short-path released,) wide-path released
    assert log[0]["op"] == "add" and log[0]["n_out"] == n
    first = [t[0] for t in steps[0][1]]
    assert first == sorted(first, reverse=True) and S.MAX_ID in first and (n < 2 or 0 in first)
    assert n < 4095 or {1, 2, 3} <= {i >> 32 for i in first}                          # job bits 1..3 mixed in
    rem = [e for e in log if e["op"] == "remove"]
    assert [e["n_out"] for e in rem] == ([n + 1] if n in S.SORT_SIZES_SHORT else [])
    fin = [e["n_out"] for e in log if e["op"] == "finish"]
    assert fin == [n if n in S.SORT_SIZES_SHORT else 0, n]
    assert (S.MAX_ID in g.ready) and (n < 2 or 0 in g.ready)                          # both ends sit in the last released list
    assert (steps[-1][0] == "payload") == (n in (4097, 8193))
    assert set(S.SORT_SIZES) == {1, 2, 3, 4095, 4096, 4097, 8191, 8192, 8193, 12289}


def test_bfs_and_blevel_depths_are_what_the_cases_say():
    assert S.BFS_CHAINS == (1, 7, 8, 9, 10, 16, 17, 18)
    for n in S.BFS_CHAINS:
        g, m, log = _played("bfs_chain", n)
        assert log[1]["n_out"] == n + 1 and log[1]["unknown"] == 0
    g, m, log = _played("bfs_diamond")
    assert log[1]["depth"] == 9 and log[2]["n_out"] == 12
    g, m, log = _played("bfs_victims")
    assert log[1]["n_out"] == 4 and log[1]["unknown"] == 1
    assert S.BLEVEL_DEPTHS == (0, 1, 8, 9, 10, 17, 18, 27)
    for d in S.BLEVEL_DEPTHS:
        g, m, log = _played("blevel_depth", d)
        assert [e["depth"] for e in log if e["op"] == "blevel"][0] == d
    assert len({len(S.blevel_shape(d)[1]) for d in S.BLEVEL_DEPTHS}) == len(S.BLEVEL_DEPTHS)


@pytest.mark.parametrize("bucket", S.CASES["hash_cluster"][1])
def test_hash_cluster_is_what_the_case_says(bucket):
    steps = S.case_hash_cluster(bucket)
    ids = [t[0] for t in steps[0][1]]
    assert len(ids) == S.CLUSTER and (S.ht_hash(ids) & (S.MIN_HASH_CAP - 1)).tolist() == [bucket] * S.CLUSTER
    assert bucket + S.CLUSTER > S.MIN_HASH_CAP or bucket == 0                         # 24 keys from bucket 8191 pass the table's end
    g, m, log = _played("hash_cluster", bucket)
    assert m.hash_rebuilds == [(0, S.MIN_HASH_CAP)]                                   # one table, never rebuilt: the tombstones stay in the cluster


def test_hash_rebuild_is_what_the_case_says():
    g, m, log = _played("hash_rebuild", 95)
    assert m.hash_rebuilds == [(0, 8192), (8192, 8192), (8192, 16384)]
    assert _adds(log)[1]["ht_used_before"] == 4000 and _adds(log)[2]["ht_used_before"] == 4095
    g, m, log = _played("hash_rebuild", 97)
    assert m.hash_rebuilds == [(0, 8192), (8192, 8192), (8192, 16384)]
    assert _adds(log)[1]["ht_used_before"] == 4000


def test_edge_pool_sums_are_what_the_case_says():
    g, m, log = _played("edge_pool", "exact")
    a = _adds(log)
    assert a[2]["edge_top_before"] + a[2]["E"] == 16384 and not a[2]["compacted"] and a[2]["cap_edges_before"] == 16384
    assert a[3]["compacted"] and m.compactions == 1
    g, m, log = _played("edge_pool", "over")
    a = _adds(log)
    assert a[2]["edge_top_before"] + a[2]["E"] == 16385 and a[2]["compacted"]
    assert a[3]["edge_top_before"] + a[3]["E"] == a[3]["cap_edges_before"] + 1 and a[3]["compacted"] and m.compactions == 2


def test_slot_cases_are_what_they_say():
    for n in (99, 100, 101):
        g, m, log = _played("slots", n)
        a = _adds(log)
        assert a[1]["free_top_before"] == 100 and a[1]["n_slots_before"] == 4096
        assert m.slot_growths == 2                                                     # the first batch, and the 2100 that pass 6144
    g, m, log = _played("rollback")
    bad = S.case_rollback()[4][1]
    assert len(bad) == 600 and bad[0][0] == bad[-1][0] and len({t[0] for t in bad}) == 599
    assert _adds(log)[1]["free_top_before"] == 100
