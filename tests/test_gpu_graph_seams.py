"""The seams of the device-resident dependency graph (csrc/graph.hip), crossed on purpose: the histories of tests/graph_seam_cases.py played on the MI355X and on
oracle/graph_oracle.py side by side.  After every step the runner compares the returned id list, the unknown count, the ready set's size, n_tasks and the
unfinished counter of EVERY id the history ever named; tests/test_graph_seam_cases.py shows without a GPU that each history builds the sizes it is named after."""
import numpy as np
import pytest

import graph_seam_cases as S
from hyperqueue_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture()
def T():
    from hyperqueue_amd.tick import Tick

    t = Tick(abi.make_config(time_limit_s=20.0))
    t.upload_ready(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    return t


def _play(T, family, arg=()):
    g, m, log = S.run(T, S.build(family, arg))
    return g, m, log


@pytest.mark.parametrize("order", S.CASES["run_lengths"][1])
def test_run_lengths(T, order):
    """A: runs of 1, 4, 5, 63..65, 4095..4097, 8192, 8193 and one of 28 875 (k_g_finish_release's SHORT_RUN and RUN_CHUNK), in both orders; then the payload"""
    _play(T, "run_lengths", order)


def test_mixed_chain_with_stale_edges(T):
    """B: a producer whose chain holds runs of 5, 4097 and 3, every 7th edge of the long one stale and its slot taken by a task that waits for somebody else"""
    _play(T, "mixed_chain")


@pytest.mark.parametrize("n", S.SORT_SIZES)
def test_sort_sizes(T, n):
    """C: output lists of exactly n entries around SORT_CH and its multiples, ids 0 and 0xFFFFFFFFFFFFFFFD among them; the payload at 4097 and 8193"""
    _play(T, "sort_size", n)


@pytest.mark.parametrize("n", S.BFS_CHAINS)
def test_recursive_removal_depth(T, n):
    """D: chains around one and two groups of BFS_LEVELS_PER_SYNC levels"""
    _play(T, "bfs_chain", n)


@pytest.mark.parametrize("family", ["bfs_diamond", "bfs_victims"])
def test_recursive_removal_claims_once(T, family):
    """D: a task reached over several paths, or named twice, leaves once"""
    _play(T, family)


@pytest.mark.parametrize("d", S.BLEVEL_DEPTHS)
def test_blevel_depth(T, d):
    """E: depths around one, two and three groups of sweeps"""
    _play(T, "blevel_depth", d)


@pytest.mark.parametrize("bucket", S.CASES["hash_cluster"][1])
def test_hash_cluster(T, bucket):
    """F: probing past tombstones, wrap-around at the last bucket, re-inserting behind tombstones"""
    _play(T, "hash_cluster", bucket)


@pytest.mark.parametrize("n_more", S.CASES["hash_rebuild"][1])
def test_hash_rebuild(T, n_more):
    """G: one key short of the rebuild rule, one key over it (in place, tombstones purged), and the growing rebuild"""
    _play(T, "hash_rebuild", n_more)


@pytest.mark.parametrize("fit", S.CASES["edge_pool"][1])
def test_edge_pool(T, fit):
    """H: edge_top + E == cap_edges leaves the pool alone, one edge more compacts it; a second compaction goes back into the first buffers"""
    _play(T, "edge_pool", fit)


@pytest.mark.parametrize("n", S.CASES["slots"][1])
def test_slots(T, n):
    """I: batches of free_top - 1, free_top and free_top + 1; then growth of the slot arrays with their contents kept"""
    _play(T, "slots", n)


def test_rollback_at_scale(T):
    """J: a refused 600-task batch on recycled slots leaves nothing behind; a finish of a waiting task is reported and carried out (existing behaviour, pinned)"""
    _play(T, "rollback")
