"""The numpy reference of the ordered view (tests/order_cases.py) against sorted() with tuple keys and plain loops, on a few hundred small sets drawn from
the key families the GPU tests use (tests/test_gpu_order_view.py).  No GPU: the reference the kernels are compared with is itself checked here."""
import numpy as np
import pytest

import order_cases as oc

TOMB = oc.TOMB


def slow_view(prio, rq):
    """the definition, one slot at a time"""
    N = len(rq)
    live = [i for i in range(N) if rq[i] != TOMB]
    perm = sorted(live, key=lambda i: (rq[i], -prio[i], i))
    inv, lrank = [TOMB] * N, [TOMB] * N
    for pos, slot in enumerate(perm):
        inv[slot] = pos
    levels = sorted({prio[i] for i in live}, reverse=True)
    where = {p: k for k, p in enumerate(levels)}
    for i in live:
        lrank[i] = where[prio[i]]
    runs = []
    for pos, slot in enumerate(perm):
        if pos == 0 or (rq[slot], prio[slot]) != (rq[perm[pos - 1]], prio[perm[pos - 1]]):
            runs.append((rq[slot], pos, lrank[slot], prio[slot]))
    return perm, inv, lrank, runs, len(levels)


def slow_mask(prio, rq):
    live = [i for i in range(len(rq)) if rq[i] != TOMB]
    if not live:
        return 0
    mask = 0
    for dg in range(12):
        vals = {((~prio[i] & oc.NONE64) >> (8 * dg)) & 0xFF if dg < 8 else (rq[i] >> (8 * (dg - 8))) & 0xFF for i in live}
        mask |= (len(vals) > 1) << dg
    return mask or 1


def draw(seed: int):
    """(prio, rq with tombstones, Q) of at most 300 slots"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 301))
    kind = seed % 8
    if kind < 6:
        prio, rq, Q = list(oc.FAMILIES.values())[kind](n, rng)
    elif kind == 6:
        dgs = sorted(rng.choice(12, int(rng.integers(1, 5)), replace=False).tolist())
        prio, rq, Q = oc.digits_vary(dgs, n, rng)
    else:
        prio, rq, Q = oc.digits_vary(list(range(12)), n, rng)
    rq = rq.copy()
    dead = rng.random(n) < [0.0, 0.1, 0.5, 0.97][seed % 4]
    rq[dead] = TOMB
    return prio, rq, Q


@pytest.mark.parametrize("block", range(8))
def test_the_reference_view_equals_the_definition(block):
    for seed in range(block * 40, block * 40 + 40):
        prio, rq, _Q = draw(seed)
        v = oc.view_reference(prio, rq)
        perm, inv, lrank, runs, n_levels = slow_view([int(x) for x in prio], [int(x) for x in rq])
        assert v.perm.tolist() == perm and v.n_live == len(perm)
        assert v.inv.tolist() == inv and v.lrank.tolist() == lrank
        assert list(zip(v.run_rq.tolist(), v.run_start.tolist(), v.run_rank.tolist(), v.run_prio.tolist())) == runs
        assert (v.n_runs, v.n_levels) == (len(runs), n_levels)
        assert v.passes == slow_mask([int(x) for x in prio], [int(x) for x in rq])


def test_digits_vary_moves_exactly_the_digits_it_names():
    rng = np.random.default_rng(1)
    for dgs in [[d] for d in range(12)] + [[2, 9], [1, 6], [3, 7, 10], [0, 5, 8, 11], list(range(12))]:
        prio, rq, Q = oc.digits_vary(dgs, 600, rng)
        assert oc.pass_mask(prio, rq) == sum(1 << d for d in dgs)
        assert int(rq.max()) < Q <= 0x01040000


def slow_select(ids, prio, rq, base, tnc, n_sel):
    perm, _inv, lrank, _runs, _L = slow_view(prio, rq)
    Q = len(tnc)
    seg = {q: [s for s in perm if rq[s] == q] for q in range(Q)}
    task, rank, slots, err = [oc.NONE64] * n_sel, [TOMB] * n_sel, [], 0
    for j in range(n_sel):
        q = max(k for k in range(Q) if base[k] <= j)
        p = j - base[q]
        if p >= len(seg[q]):
            err = 1
            continue
        slot, dst = seg[q][p], j
        nw, c = tnc[q] >> 16, tnc[q] & 0xFFFF
        if tnc[q] and p < nw * c:
            sw = p // nw
            dst = base[q] + (p - sw * nw) * c + sw
        task[dst], rank[dst] = ids[slot], lrank[slot]
        slots.append(slot)
    return task, rank, slots, err


@pytest.mark.parametrize("block", range(4))
def test_the_reference_selection_equals_the_definition(block):
    for seed in range(block * 25, block * 25 + 25):
        rng = np.random.default_rng(1000 + seed)
        prio, rq, Q = draw(seed * 8 + int(rng.integers(0, 6)))   # (the families with a handful of requests)
        ids = oc.make_ids(len(rq))
        v = oc.view_reference(prio, rq)
        have = np.bincount(rq[rq != TOMB], minlength=Q)
        take = np.minimum(have, rng.integers(0, 12, Q))
        take[rng.random(Q) < 0.3] = 0                              # requests that take nothing share their base with the next one
        over = seed % 5 == 0 and take.sum() > 0
        if over:                                                  # one task more than a segment holds: the guard
            q = int(rng.choice(np.flatnonzero(take)))
            take[q] = have[q] + 1
        tnc = np.zeros(Q, np.int64)
        for q in range(Q):
            t = int(take[q])
            if t >= 2 and rng.random() < 0.6 and not (over and t > have[q]):
                nw = int(rng.integers(1, t + 1))
                tnc[q] = nw << 16 | (t // nw)                      # nw * c <= take: the tail keeps dst = j
        base = np.concatenate([[0], np.cumsum(take)])
        n_sel = int(base[-1])
        if n_sel == 0:
            continue
        task, rank, slots, err = oc.select_reference(ids, v, base, tnc, n_sel)
        s_task, s_rank, s_slots, s_err = slow_select([int(x) for x in ids], [int(x) for x in prio], [int(x) for x in rq], base.tolist(), tnc.tolist(), n_sel)
        assert task.tolist() == s_task and rank.tolist() == s_rank and sorted(slots.tolist()) == sorted(s_slots) and err == s_err == int(over)


def test_the_reference_rank_of_equals_the_definition():
    for seed in range(60):
        prio, rq, _Q = draw(seed)
        ids = oc.make_ids(len(rq))
        v = oc.view_reference(prio, rq)
        rng = np.random.default_rng(seed)
        want = np.concatenate([ids[rng.integers(0, len(ids), 20)], rng.integers(0, int(ids[-1]) + 9, 20).astype(np.uint64), [0, ids[0], ids[-1], ids[-1] + 1]]).astype(np.uint64)
        got_rq, got_pos = oc.rank_of_reference(ids, rq, v, want)
        where = {int(t): i for i, t in enumerate(ids)}
        for k, w in enumerate(want.tolist()):
            i = where.get(w)
            if i is None or rq[i] == TOMB:
                assert (got_rq[k], got_pos[k]) == (TOMB, TOMB)
            else:
                assert (got_rq[k], got_pos[k]) == (rq[i], v.perm.tolist().index(i))
