"""Mid-size coupled ticks whose worker blocks are NOT packings (a helper module of the suite, not a conftest).

tools/price_fuzz.py's `scenario(seed)` gives a cluster mid-run whose placement model couples all workers; every worker's block there is a packing (`<=` resource
rows with non-negative coefficients over columns with lower bound 0).  The variants below add what `workloads` / `core` already model:

  mu       min_utilization from {0.3, 0.6, 1.0} on a random 30-80 % of the workers: the builder's add_min_utilization pair (`cpu.x - need*y >= 0`,
           `cpu.x - all*y <= 0`, a zero-cost bool y) lands INSIDE the worker's block — the block is no longer a packing
  mu6      the same with min_utilization 0.6 on each worker whose draw is below 0.7: the draw on which the block-hull cuts were first seen to certify a
           fraction of the optimum (seeds 2005, 2014 and 2017)
  mn       a multi-node request over worker groups: a share of the workers is idle (the MN batch needs free workers), each group's MN placement columns tied
           to a group column by an `==` row.  The group column belongs to no block, so that row couples blocks; the worker blocks stay packings
  blocked  blocked (worker, request, variant) triples: blocker flag columns carry part of the objective.  The flags belong to no block either: coupling rows
           with a cost, worker blocks still packings (these ticks may go to the price sweeps)
  mixed    mu, mn and blocked together: non-packing blocks under coupling rows of every kind

So mu, mu6 and mixed exercise the block classification of csrc/milp.cpp (find_hull_blocks); mn and blocked exercise the rest of the solve and the mapping.

Every case must give a model of >= 128 columns and carry what its variant is about (`case_model` asserts both): a case that shrinks or loses its rows fails
instead of quietly testing less.  SEEDS are the committed lists per variant: the first 24 seeds from 2000 up whose model qualifies and has at most 600
columns (the root cut passes of csrc/milp.cpp, block-hull cuts among them, run on models up to that size; above it a case costs its full time limit and tests
no cut); for mu6 the three seeds above.  On 10 mu cases, the 3 mu6 cases and 11 mixed ones the block-hull cuts used to certify up to 64 % below the optimum.
GPU_SEEDS is the subset the GPU suite runs.
"""
from __future__ import annotations

import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from hyperqueue_amd import abi  # noqa: E402
from hyperqueue_amd.core import FR  # noqa: E402

VARIANTS = ("mu", "mu6", "mn", "blocked", "mixed")
MIN_COLS, MAX_COLS = 128, 600

SEEDS = {
    "mu6": [2005, 2014, 2017],
    "mu": [2000, 2005, 2006, 2007, 2010, 2013, 2014, 2016, 2017, 2018, 2019, 2023, 2024, 2025, 2027, 2028, 2029, 2031, 2032, 2034, 2035, 2036, 2040, 2041],
    "mn": [2000, 2005, 2006, 2007, 2013, 2014, 2016, 2017, 2018, 2019, 2023, 2024, 2025, 2027, 2028, 2029, 2031, 2032, 2034, 2035, 2036, 2040, 2041, 2043],
    "blocked": [2000, 2005, 2006, 2007, 2014, 2016, 2017, 2018, 2024, 2025, 2028, 2029, 2031, 2032, 2036, 2040, 2041, 2043, 2044, 2046, 2047, 2050, 2051, 2052],
    "mixed": [2000, 2005, 2006, 2007, 2013, 2014, 2016, 2017, 2018, 2019, 2023, 2024, 2025, 2027, 2028, 2029, 2031, 2032, 2034, 2035, 2036, 2041, 2043, 2044],
}
GPU_SEEDS = {
    "mu6": [2005, 2014, 2017],
    "mu": [2000, 2005, 2007, 2014, 2017, 2019, 2032, 2041],
    "mn": [2000, 2005, 2006, 2007, 2013, 2014, 2017, 2018],
    "blocked": [2000, 2005, 2006, 2007, 2014, 2016, 2017, 2024],
    "mixed": [2000, 2005, 2006, 2007, 2013, 2017, 2018, 2043],
}


def _min_utilization(snap, rng):
    W = len(snap.worker_id)
    u = rng.random(W)
    frac = 0.3 + 0.5 * rng.random()
    vals = np.asarray([0.3, 0.6, 1.0])[rng.integers(0, 3, W)]
    snap.worker_min_utilization = np.where(u < frac, vals, 0.0).astype(np.float32)


def _min_utilization_06(snap, rng):
    W = len(snap.worker_id)
    snap.worker_min_utilization = np.where(rng.random(W) < 0.7, 0.6, 0.0).astype(np.float32)


def _multi_node(snap, rng):
    """one multi-node request (2-4 nodes) with a few ready tasks at a random existing priority, workers in 2-4 groups, 25-50 % of them idle"""
    W = len(snap.worker_id)
    idle = rng.random(W) < 0.25 + 0.25 * rng.random()
    idle[int(rng.integers(0, W))] = True
    for w in np.nonzero(idle)[0]:
        snap.worker_free[w] = snap.worker_total[w]
        snap.assigned[w] = []
    G = int(rng.integers(2, 5))
    snap.worker_group = rng.integers(0, G, W).astype(np.uint32)
    snap.n_groups = G
    k = int(rng.integers(2, 5))
    snap.requests = list(snap.requests) + [[dict(entries=[(0, abi.HQ_ENTRY_AMOUNT, FR)], n_nodes=k, min_time_ns=0, weight=10_000)]]
    rq = len(snap.requests) - 1
    n_mn = int(rng.integers(1, 1 + max(1, int(idle.sum()) // k)))
    last = int(snap.task_id.max()) if len(snap.task_id) else 1 << 32
    prio = snap.task_priority[rng.integers(0, len(snap.task_priority), n_mn)] if len(snap.task_priority) else np.zeros(n_mn, np.uint64)
    snap.task_id = np.concatenate([snap.task_id, np.arange(last + 1, last + 1 + n_mn, dtype=np.uint64)])
    snap.task_priority = np.concatenate([snap.task_priority, np.asarray(prio, np.uint64)])
    snap.task_rq = np.concatenate([snap.task_rq, np.full(n_mn, rq, np.uint32)])


def _blocked(snap, rng):
    """each of 10-40 % of the workers blocks one or two of the single-node requests of the ready set (variant 0)"""
    W = len(snap.worker_id)
    sn_rqs = sorted({int(q) for q in np.unique(snap.task_rq) if all(v["n_nodes"] == 0 for v in snap.requests[int(q)])})
    frac = 0.1 + 0.3 * rng.random()
    out = set()
    for w in range(W):
        if rng.random() < frac and sn_rqs:
            for q in rng.choice(sn_rqs, size=min(len(sn_rqs), int(rng.integers(1, 3))), replace=False):
                out.add((w, int(q), 0))
    snap.blocked = sorted(out)


def case(variant: str, seed: int) -> abi.Snapshot:
    """the snapshot of one case: price_fuzz.scenario(seed) with the variant's changes, each drawn from its own generator"""
    from price_fuzz import scenario

    assert variant in VARIANTS, variant
    snap = scenario(seed)[0]
    if variant in ("mu", "mixed"):
        _min_utilization(snap, np.random.default_rng(seed + 7))
    if variant == "mu6":
        _min_utilization_06(snap, np.random.default_rng(seed + 7))
    if variant in ("mn", "mixed"):
        _multi_node(snap, np.random.default_rng(seed + 11))
    if variant in ("blocked", "mixed"):
        _blocked(snap, np.random.default_rng(seed + 13))
    return snap


def case_model(variant: str, snap: abi.Snapshot) -> dict:
    """the oracle's placement model of the snapshot (built, not solved: the tick is given no counts), asserted to be of the family's size and to hold the
    variant's non-packing structure: min_utilization pairs (`>=` rows), multi-node group rows (`==` rows), flag columns with a cost"""
    from oracle.oracle import Oracle

    o = Oracle(abi.make_config(time_limit_s=1.0))
    o.tick_given(snap, [], is_optimal=False)
    m = o.last_model()
    n = len(m["obj"])
    assert MIN_COLS <= n <= MAX_COLS, f"the case's model has {n} columns, outside the family's {MIN_COLS}..{MAX_COLS}"
    if variant in ("mu", "mu6", "mixed"):
        assert _has_min_utilization(m), "no min_utilization row in the model"
    if variant in ("mn", "mixed"):
        assert (m["rtype"] == 2).any(), "no multi-node group row in the model"
    if variant in ("blocked", "mixed"):
        assert flags_carry_objective(m), "no flag column with a cost in the model"
    return m


def model_digest(m: dict) -> str:
    """SHA-256 over the model's objective, column kinds and rows: a pin computed on another model must not be compared against"""
    import hashlib

    h = hashlib.sha256()
    for k in ("obj", "kind", "ctype", "rtype", "rhs", "roff", "rcol", "rcoef"):
        a = np.ascontiguousarray(m[k])
        h.update(k.encode())
        h.update(str(a.dtype).encode())
        h.update(np.asarray(a.shape, np.int64).tobytes())
        h.update(a.tobytes())
    return h.hexdigest()


def _has_min_utilization(m: dict) -> bool:
    """a `>=` row with a negative coefficient: `cpu.x - need*y >= 0` (priority cuts and blocker rows have none)"""
    for i in np.nonzero(m["rtype"] == 0)[0]:
        if (m["rcoef"][m["roff"][i]:m["roff"][i + 1]] < 0).any():
            return True
    return False


def flags_carry_objective(m: dict) -> bool:
    return any(m["ctype"][j] != 0 and m["obj"][j] != 0 for j in range(len(m["obj"])))


def host_solve(variant: str, seed: int, time_limit_s: float = 5.0) -> dict:
    """one case through the product's host stages (tests/host_stages.HostStages: the tick's batches and solver on the scan outputs computed in numpy)"""
    from host_stages import HostStages

    snap = case(variant, seed)
    hs = HostStages(abi.make_config(time_limit_s=time_limit_s))
    r = hs.stages(snap)
    mn = last_mn(hs.lib)
    return dict(status=int(r.status), is_optimal=bool(r.is_optimal), is_canonical=bool(r.is_canonical), counts=[list(map(int, c)) for c in r.counts],
                batches=[[b.rq, b.size] for b in r.batches], mn=mn)


def last_mn(lib) -> list:
    """the multi-node placements of the last host-stages call on this thread (hqtick_debug_last_mn; the counts carry single-node placements only):
    (request, [worker indices]) per placed multi-node task"""
    import ctypes as C

    u32pp = C.POINTER(C.POINTER(C.c_uint32))
    lib.hqtick_debug_last_mn.argtypes = [u32pp, u32pp, u32pp]
    lib.hqtick_debug_last_mn.restype = C.c_uint32
    rq, off, wk = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
    k = lib.hqtick_debug_last_mn(C.byref(rq), C.byref(off), C.byref(wk))
    return [[int(rq[i]), [int(wk[j]) for j in range(off[i], off[i + 1])]] for i in range(k)]


def mn_placements(snap, res) -> list:
    """an abi.Result's multi-node tasks as (request, [worker indices]), the shape host_solve gives"""
    rq_of = {int(t): int(q) for t, q in zip(snap.task_id, snap.task_rq)}
    return [[rq_of[int(t)], [int(w) for w in ws]] for (t, ws) in res.mn]


def host_solve_fresh(variant: str, seed: int, hull_cuts: bool = True, time_limit_s: float = 5.0, env: dict | None = None):
    """host_solve in a fresh Python process: csrc/milp.cpp reads HQMILP_HULL_CUTS once, in a static initialiser, so a solve with the block-hull cuts off
    needs a process of its own.  Returns the subprocess.Popen whose stdout is the JSON of host_solve; `read_fresh` collects it."""
    import subprocess

    e = dict(os.environ if env is None else env)
    e["HQMILP_HULL_CUTS"] = "1" if hull_cuts else "0"
    e["HIP_VISIBLE_DEVICES"] = e["ROCR_VISIBLE_DEVICES"] = "-1"   # the host stages never open a device: make sure no child can
    code = f"import coupled_cases as cc, json; print(json.dumps(cc.host_solve({variant!r}, {int(seed)}, {float(time_limit_s)!r})))"
    return subprocess.Popen([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True)


def read_fresh(p, timeout_s: float = 120.0) -> dict:
    import json

    out, err = p.communicate(timeout=timeout_s)
    assert p.returncode == 0, f"solve process failed ({p.returncode}): {err[-2000:]}"
    return json.loads(out.strip().splitlines()[-1])
