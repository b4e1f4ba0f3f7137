"""The non-packing coupled family (tests/coupled_cases.py) through the HIP tick (hyperqueue_amd.tick.Tick, C ABI) — GPU only.

1. Soundness, feasibility and agreement against the exact oracle's pins (tests/golden/nonpacking/coupled_nonpacking.json), as in
   tests/test_solver_nonpacking.py.  No HiGHS solve of the placement runs here: HiGHS only completes the flag columns of the GPU's fixed placement (single-
   and multi-node) to check its rows and price it.  The price path refuses blocks that are not packings (csrc/price.cpp), so the mu / mu6 / mixed ticks are
   solved by the host branch-and-cut that libhqtick.so links: the same csrc/milp.cpp whose block-hull cuts used to certify a fraction of the optimum.
2. The device stages against their emulation: K1's level scan, K2's eligibility rows and the K4/K5 mapping on mid-size clusters with min_utilization,
   worker groups with a multi-node request and blocked requests.  When the GPU tick and the host stages (price sweeps on the emulated wavefront) both return
   a canonical answer, batches, counts and multi-node placements are identical.  The records, retracts, redirects, multi-node tasks and free vectors are the
   oracle's mapping of the GPU's placement, the multi-node one included.
3. Which ticks ran price sweeps, pinned: a case whose blocks are all packings may go to the sweeps, the others may not.

One process, the cases in sequence, nothing retried.
"""
import pytest

import coupled_cases as cc
from hyperqueue_amd import abi

pytestmark = pytest.mark.gpu

CASES = [(v, s) for v in cc.VARIANTS for s in cc.GPU_SEEDS[v]]
# The cases whose tick runs price sweeps (kernel_stats()["price_sweeps"] > 0), as the emulation and the MI355X both count them: none wherever a block is
# not a packing (min_utilization) or a multi-node request is in the model; some of the blocked cases, whose blocks are all packings.  The count itself must
# equal the emulation's when both sides are canonical.
SWEPT = {"blocked": {2007, 2014, 2017}}


def _emulated(snap):
    from test_price import stages

    got, sweeps, _ = stages(snap, True, min_cols=0, tl=5.0)
    return got, sweeps


@pytest.mark.parametrize("variant,seed", CASES)
def test_gpu_case(variant, seed):
    from hyperqueue_amd.tick import Tick
    from test_solver_nonpacking import check_case, pins

    snap = cc.case(variant, seed)
    t = Tick(abi.make_config(time_limit_s=5.0))
    try:
        got = t.tick(snap)
        ks = t.kernel_stats()
    finally:
        t.close()
    assert got.status in (abi.HQTICK_DONE, abi.HQTICK_NEED_MORE_COMPUTE), got.status
    m = cc.case_model(variant, snap)
    mn = cc.mn_placements(snap, got)
    check_case(variant, seed, got, pins()[f"{variant}/{seed}"], m, mn=mn)
    # parity tier T3 on the GPU's placement: the single-node counts plus one count per worker of each placed multi-node task (the oracle's MN placement
    # columns, keyed like the single-node ones by (request, variant 0, worker)) given to the oracle; its decode + mapping + prefill (Oracle.tick_given) must
    # give the GPU's records, retracts, redirects, multi-node tasks and free vectors
    from oracle.oracle import Oracle

    given = list(got.counts) + [(q, 0, w, 1) for (q, ws) in mn for w in ws]
    want = Oracle(abi.make_config(time_limit_s=5.0)).tick_given(snap, given, is_optimal=bool(got.is_optimal))
    assert got.batches == want.batches and got.counts == want.counts
    assert got.mn == want.mn
    assert got.records == want.records and got.retracts == want.retracts and sorted(got.redirects) == sorted(want.redirects)
    assert (got.new_free == want.new_free).all()
    emu, emu_sweeps = _emulated(snap)
    if got.is_canonical and emu.is_canonical:
        from hyperqueue_amd import _testhooks

        emu_mn = cc.last_mn(_testhooks.load())
        assert got.batches == emu.batches and got.counts == emu.counts, f"{variant}/{seed}: the device stages and their emulation differ"
        assert sorted((q, sorted(ws)) for q, ws in mn) == sorted((q, sorted(ws)) for q, ws in emu_mn), (variant, seed, mn, emu_mn)
    sweeps = int(ks["price_sweeps"])
    assert (sweeps > 0) == (emu_sweeps > 0) == (seed in SWEPT.get(variant, ())), (variant, seed, sweeps, emu_sweeps)
    if got.is_canonical and emu.is_canonical:
        assert sweeps == emu_sweeps, (variant, seed, sweeps, emu_sweeps)
