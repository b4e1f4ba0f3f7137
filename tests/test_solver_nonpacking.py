"""Coupled-tick certificates on worker blocks that are NOT packings (tests/coupled_cases.py: min_utilization, multi-node groups, blocked requests), against
the exact oracle's pinned answers (tests/golden/nonpacking/coupled_nonpacking.json) — and the solver on small block models against exact enumeration.

`is_optimal = 1` claims the objective is within 1e-4 of the optimum.  The block-hull cuts of csrc/milp.cpp (hull_round) used to hold every column with a
non-positive Lagrangian cost at 0 in the block solve, which is valid only for down-closed blocks: on a worker with min_utilization the pair's zero-cost bool
went to 0, the block's value to ~0, and the cut removed every point that uses the worker — certified at a fraction of the optimum.
"""
import ctypes as C
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import coupled_cases as cc
from hyperqueue_amd import abi
from limits import completed_point, rows_hold

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nonpacking", "coupled_nonpacking.json")
CASES = [(v, s) for v in cc.VARIANTS for s in cc.SEEDS[v]]
REL = 1e-4


def pins():
    with open(PINS) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def solved():
    """every case solved twice in fresh processes — block-hull cuts on and off (HQMILP_HULL_CUTS is read once per process) — several at a time"""
    par = max(1, min(6, (os.cpu_count() or 2) // 2))
    out = {}

    def run(key):
        v, s, hull = key
        return key, cc.read_fresh(cc.host_solve_fresh(v, s, hull_cuts=hull, time_limit_s=5.0))

    with ThreadPoolExecutor(par) as ex:
        for key, r in ex.map(run, [(v, s, h) for (v, s) in CASES for h in (True, False)]):
            out[key] = r
    return out


def check_case(variant, seed, got, pin, model=None, mn=None):
    """soundness, feasibility and agreement of one product answer against the pin; returns z_product.  `got` is host_solve's dict (its "mn" the host
    stages' multi-node placements) or an abi.Result with `mn` = coupled_cases.mn_placements of it."""
    snap = cc.case(variant, seed)
    m = model if model is not None else cc.case_model(variant, snap)
    assert (len(m["obj"]), len(m["rhs"])) == (pin["cols"], pin["rows"]) and cc.model_digest(m) == pin["digest"], \
        f"{variant}/{seed}: the model is not the one the pin was computed on (regenerate tests/golden/nonpacking/coupled_nonpacking.json)"
    counts = [tuple(c) for c in (got["counts"] if isinstance(got, dict) else got.counts)]
    is_opt = bool(got["is_optimal"] if isinstance(got, dict) else got.is_optimal)
    mn = got["mn"] if isinstance(got, dict) else mn
    assert mn is not None
    # feasibility: the product's single-node counts AND multi-node placements fixed, only the flag columns (and the group counts the fixed placements imply)
    # left to choose, every row of the oracle's model holds; no batch places more tasks than it has ready
    out = completed_point(m, counts, mn=mn)
    assert out is not None, f"{variant}/{seed}: the product's placement violates a row of the oracle's model"
    x = out[0]
    assert rows_hold(m, x), f"{variant}/{seed}: the product's placement violates a row of the oracle's model"
    ready = np.bincount(np.asarray(snap.task_rq, np.int64), minlength=len(snap.requests))
    batches = got["batches"] if isinstance(got, dict) else [[b.rq, b.size] for b in got.batches]
    for b in batches:
        assert b[1] <= ready[b[0]], (variant, seed, b[:2], int(ready[b[0]]))
    per_rq = {}
    for (q, _v, _w, c) in counts:
        per_rq[q] = per_rq.get(q, 0) + c
    for q, ws in mn:
        per_rq[q] = per_rq.get(q, 0) + 1
        assert len(ws) == snap.requests[q][0]["n_nodes"] and len(set(ws)) == len(ws), (variant, seed, q, ws)
    for q, c in per_rq.items():
        assert c <= ready[q], (variant, seed, q, c, int(ready[q]))
    z = float(np.dot(m["obj"], x))
    zo = pin["objective"]
    # soundness: a certificate is never below the best point the oracle verified (proved optimal or not)
    if is_opt:
        assert z >= zo - REL * abs(zo), f"{variant}/{seed}: certified {z:.9f}, the oracle's verified point reaches {zo:.9f}"
    # agreement: two proofs name the same optimum
    if is_opt and pin["proved_optimal"]:
        assert abs(z - zo) <= REL * abs(zo), f"{variant}/{seed}: certified {z:.9f}, oracle proved {zo:.9f}"
    return z


def test_pins_cover_the_family():
    p = pins()
    assert sorted(p) == sorted(f"{v}/{s}" for v, s in CASES)


@pytest.mark.parametrize("variant,seed", CASES)
def test_case_soundness(variant, seed, solved):
    pin = pins()[f"{variant}/{seed}"]
    snap = cc.case(variant, seed)
    m = cc.case_model(variant, snap)
    on, off = solved[(variant, seed, True)], solved[(variant, seed, False)]
    assert on["status"] in (abi.HQTICK_DONE, abi.HQTICK_NEED_MORE_COMPUTE) and off["status"] in (abi.HQTICK_DONE, abi.HQTICK_NEED_MORE_COMPUTE)
    z_on = check_case(variant, seed, on, pin, m)
    z_off = check_case(variant, seed, off, pin, m)
    # an invalid cut shows without HiGHS: the search without block-hull cuts must not find a point above a certificate that rests on them
    if on["is_optimal"]:
        assert z_off <= z_on + REL * abs(z_on), f"{variant}/{seed}: certified {z_on:.9f} with block-hull cuts, {z_off:.9f} found without them"


@pytest.mark.parametrize("key", ["mu/2019", "mn/2000", "mixed/2013"])
def test_pin_reproduces_live(key):
    """the exact oracle, re-run: same model, same best verified objective"""
    from oracle.oracle import Oracle

    v, s = key.split("/")
    pin = pins()[key]
    o = Oracle(abi.make_config(time_limit_s=60.0))
    r = o.tick(cc.case(v, int(s)))
    m = o.last_model()
    assert cc.model_digest(m) == pin["digest"]
    z = float(np.dot(m["obj"], m["x"]))
    assert bool(r.is_optimal) == pin["proved_optimal"]
    assert abs(z - pin["objective"]) <= 1e-9 * max(1.0, abs(pin["objective"])), (z, pin["objective"])


# ---- small block models against exact enumeration ---------------------------------------------------------------------------------------------------------
# Shaped like a coupled tick: blocks of 4-8 integer columns (one per worker: col_group) with a cpu row, sometimes a memory row and per-column caps, and in some
# blocks the min_utilization pair over a zero-cost bool; one or two wide rows with coefficients 1-2 across all blocks.  18-28 blocks: from 128 columns on the
# solver runs its root cut rounds — the block-hull pass among them — before the window search; a model of a handful of blocks closes in its first dive and
# never reaches a hull round.  Every coefficient and cost is a small integer, so the enumeration below is exact.

def small_model(seed):
    rng = np.random.default_rng(seed)
    B = int(rng.integers(18, 29))
    obj, kind, group, rows = [], [], [], []   # rows: (type, rhs, [(col, coef)])
    for b in range(B):
        k = int(rng.integers(4, 9))
        cols = list(range(len(obj), len(obj) + k))
        cpu = rng.integers(1, 5, k)
        for _ in range(k):
            obj.append(int(rng.integers(1, 31))); kind.append(0); group.append(b)
        CPU = int(rng.integers(4, 11))
        rows.append((1, CPU, [(cols[j], int(cpu[j])) for j in range(k)]))
        if rng.random() < 0.6:
            mem = rng.integers(0, 4, k)
            rows.append((1, int(rng.integers(2, 8)), [(cols[j], int(mem[j])) for j in range(k) if mem[j]]))
        for j in range(k):
            if rng.random() < 0.5:
                rows.append((1, int(rng.integers(1, 4)), [(cols[j], 1)]))
        if rng.random() < 0.6:   # cpu.x - need*y >= 0, cpu.x - all*y <= 0, y a zero-cost bool (host_model.cpp add_min_utilization)
            y = len(obj); obj.append(0); kind.append(1); group.append(b)
            need = int(rng.integers(2, CPU + 1))
            rows.append((0, 0, [(cols[j], int(cpu[j])) for j in range(k)] + [(y, -need)]))
            rows.append((1, 0, [(cols[j], int(cpu[j])) for j in range(k)] + [(y, -CPU)]))
    n = len(obj)
    for _ in range(int(rng.integers(1, 3))):
        terms = [(j, int(rng.integers(1, 3))) for j in range(n) if kind[j] == 0 and rng.random() < 0.7]
        rows.append((1, int(rng.integers(len(terms) // 6, len(terms) // 3)), terms))
    return np.asarray(obj, np.int64), np.asarray(kind, np.uint8), np.asarray(group, np.int32), rows


def exact_optimum(obj, kind, group, rows):
    """max c.x by enumeration: every block's integer points (each column bounded by its block's cpu row, coefficients >= 1), reduced to the best value per
    vector of wide-row activities, then a DP over the blocks on those activities (the wide rows are `<=` with non-negative coefficients)"""
    n = len(obj)
    wide = [r for r in rows if len({int(group[j]) for j, _ in r[2]}) > 1]
    assert all(r[0] == 1 and all(a >= 0 for _, a in r[2]) for r in wide)
    cap = np.asarray([r[1] for r in wide], np.int64)
    dp = np.full(tuple(cap + 1), -1, np.int64)
    dp[(0,) * len(wide)] = 0
    for b in sorted(set(group.tolist())):
        cols = [j for j in range(n) if group[j] == b]
        own = [r for r in rows if r not in wide and all(group[j] == b for j, _ in r[2])]
        cpu_row = own[0]
        pos = {j: i for i, j in enumerate(cols)}
        ub = [1 if kind[j] == 1 else cpu_row[1] // dict(cpu_row[2])[j] for j in cols]
        pts = np.zeros((1, 0), np.int64)
        for i in range(len(cols)):
            pts = np.repeat(pts, ub[i] + 1, axis=0)
            pts = np.concatenate([pts, np.tile(np.arange(ub[i] + 1), len(pts) // (ub[i] + 1))[:, None]], axis=1)
            part = sum(a * pts[:, pos[j]] for j, a in cpu_row[2] if pos[j] <= i)
            pts = pts[part <= cpu_row[1]]
        ok = np.ones(len(pts), bool)
        for (t, rhs, terms) in own:
            act = sum(a * pts[:, pos[j]] for j, a in terms)
            ok &= (act <= rhs) if t == 1 else (act >= rhs) if t == 0 else (act == rhs)
        pts = pts[ok]
        val = pts @ obj[cols]
        acts = np.stack([sum(a * pts[:, pos[j]] for j, a in terms if j in pos) if any(j in pos for j, _ in terms) else np.zeros(len(pts), np.int64)
                         for (_, _, terms) in wide], axis=1)
        best = {}
        for a, v in zip(map(tuple, acts), val):
            if all(x <= c for x, c in zip(a, cap)) and best.get(a, -1) < v:
                best[a] = int(v)
        new = np.full(dp.shape, -1, np.int64)
        for a, v in best.items():
            src = dp[tuple(slice(0, c + 1 - x) for x, c in zip(a, cap))]
            dst = new[tuple(slice(x, c + 1) for x, c in zip(a, cap))]
            np.maximum(dst, np.where(src >= 0, src + v, -1), out=dst)
        dp = new
    return int(dp.max())


def solve_priced(obj, kind, group, rows, time_limit_s=5.0):
    from hyperqueue_amd import _testhooks

    lib = _testhooks.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    n, m = len(obj), len(rows)
    objf = np.asarray(obj, float)
    rtype = np.asarray([r[0] for r in rows], np.uint8); rhs = np.asarray([r[1] for r in rows], float)
    roff = np.cumsum([0] + [len(r[2]) for r in rows]).astype(np.int32)
    rcol = np.asarray([t[0] for r in rows for t in r[2]], np.int32); rcoef = np.asarray([t[1] for r in rows for t in r[2]], float)
    x, z, opt = np.zeros(n), C.c_double(), C.c_int()
    lib.hqtick_debug_milp_solve_priced.restype = C.c_int
    ok = lib.hqtick_debug_milp_solve_priced(C.c_int(n), objf.ctypes.data_as(dp), kind.ctypes.data_as(abi.u8p), group.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(m),
                                            rtype.ctypes.data_as(abi.u8p), None, rhs.ctypes.data_as(dp), roff.ctypes.data_as(ip), rcol.ctypes.data_as(ip),
                                            rcoef.ctypes.data_as(dp), C.c_double(time_limit_s), C.c_int(0), C.c_uint32(0), x.ctypes.data_as(dp), C.byref(z),
                                            C.byref(opt), None)
    hs, hn = C.c_long(), C.c_long()
    lib.hqtick_debug_milp_last_hull.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    lib.hqtick_debug_milp_last_hull(C.byref(hs), C.byref(hn))
    return bool(ok), x, z.value, bool(opt.value), hs.value, hn.value


SMALL_SEEDS = range(40)


def test_small_block_models_exact():
    """certified objective == the enumerated maximum (1e-9 relative), x satisfies every row; and the block-hull round ran on non-packing blocks"""
    hull_nonpacking = []
    for seed in SMALL_SEEDS:
        obj, kind, group, rows = small_model(seed)
        ok, x, z, opt, hs, hn = solve_priced(obj, kind, group, rows)
        assert ok, seed
        assert np.all(x >= 0) and np.all(x == np.round(x)) and np.all(x[kind == 1] <= 1), seed
        for (t, rhs, terms) in rows:
            act = sum(a * x[j] for j, a in terms)
            assert (act <= rhs + 1e-9) if t == 1 else (act >= rhs - 1e-9) if t == 0 else abs(act - rhs) <= 1e-9, (seed, t, rhs, act)
        assert abs(z - float(np.dot(obj, x))) <= 1e-9 * max(1.0, abs(z)), seed
        want = exact_optimum(obj, kind, group, rows)
        assert z <= want + 1e-9 * want, (seed, z, want)
        if opt:
            assert abs(z - want) <= 1e-9 * want, f"seed {seed}: certified {z}, the enumerated maximum is {want}"
        if hn:
            hull_nonpacking.append(seed)
    # the proof that this test reaches what it is about: block-hull solves on blocks that are not packings (hull_round's counter, milp.cpp)
    assert len(hull_nonpacking) >= 2, hull_nonpacking
