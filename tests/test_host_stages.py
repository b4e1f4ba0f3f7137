"""The tick's HOST stages (batches + placement: separable path, lazy size rows, empty-worker elimination, exact solver) on a machine
without a GPU, through hqtick_debug_host_stages: same batches and same counts as the canonical oracle on the randomised scenario
families of the GPU fuzz suite — and, through hqtick_debug_host_plan, the host part of the mapping (csrc/map_core.h: retracts, redirects with their
kinds, free vectors, records per worker) equal to the reference's mapping on the same placement (Oracle.tick_given).  (The scan kernels, the selection and
the records themselves run only on the GPU: tests/test_gpu_*.py.)"""
import numpy as np
import pytest

from host_stages import HostStages
from hyperqueue_amd import abi
from hyperqueue_amd.core import TaskBuilder as TB


def _objective(model, res):
    """c.x of a result's counts in the oracle's model of the same snapshot (placement columns only: flag columns cost nothing)"""
    cd = {(q, v, w): c for (q, v, w, c) in res.counts}
    x = np.zeros(len(model["obj"]))
    for j in range(len(x)):
        if model["ctype"][j] == 0:
            x[j] = cd.get((int(model["crq"][j]), int(model["cvariant"][j]), int(model["cworker"][j])), 0)
    return float(np.dot(model["obj"], x))


def _completed_objective(model, res):
    """c.x of a result's counts completed with the best values of the model's other columns (flag columns of blocked workers carry part of the objective,
    and the hook exports placement counts only): the placement columns fixed, HiGHS picks the rest"""
    from limits import completed_point

    out = completed_point(model, res.counts)
    assert out is not None, "the placement counts admit no completion: infeasible point"
    return out[1]


def _same_host_part(got, want, model):
    assert got.status == want.status and got.is_optimal == want.is_optimal
    assert got.batches == want.batches
    if got.is_canonical or not got.is_optimal:
        assert got.counts == want.counts
    else:  # optimal in the reference's sense (certified within HiGHS's default mip_rel_gap = 1e-4) but not canonical (hqtick_result.is_canonical = 0:
        # the exact pass or the tie-break phase ran out of its budget): the claim is the objective value, within that gap of the exact oracle's
        if any(model["ctype"][j] != 0 and model["obj"][j] > 0 for j in range(len(model["obj"]))):
            return  # multi-node columns carry part of the objective and the hook exports single-node counts only: nothing to compare here
        zg, zw = _objective(model, got), _objective(model, want)
        assert zw * (1.0 - 1e-4) - 1e-12 <= zg <= zw + 1e-9 * max(1.0, abs(zw)), (zg, zw)


MAPPING_ASSERTS = "a Retracting task reached take_tasks_for_prefill: the reference asserts task.is_waiting() (mapping.rs:221)"


def _same_mapping_part(hs, snap):
    """The host part of the mapping on this snapshot (hqtick_debug_host_plan) against the reference's mapping on the SAME placement (Oracle.tick_given on the
    hook's counts and multi-node placements, which needs no solver and so is never skipped for a solver's limit): per-worker retracts, redirects with their
    kinds, new_free, and the number of records of every worker — what test_gpu_parity.assert_same compares, minus what needs K4 / K5.  Where the reference
    asserts (a Retracting task reaching take_tasks_for_prefill), the hook must refuse with HQTICK_E_UNSUPPORTED and that text.  Returns the reference's
    result, or None where it asserts."""
    import coupled_cases as cc
    from hyperqueue_amd import tick
    from oracle.oracle import Oracle

    got = refusal = None
    try:
        got, rec_off = hs.plan(snap)
        base = got
    except tick.HqTickError as e:
        refusal = e
        base = hs.stages(snap)  # (the same body without the plan: the placement the refused plan was made for)
    given = list(base.counts) + [(q, 0, w, 1) for (q, ws) in cc.last_mn(hs.lib) for w in ws]
    try:
        want = Oracle(hs.cfg, canonical=True).tick_given(snap, given, base.is_optimal)
    except RuntimeError:
        assert refusal is not None and refusal.code == abi.HQTICK_E_UNSUPPORTED and MAPPING_ASSERTS in str(refusal), refusal
        return None
    assert refusal is None, refusal
    assert got.counts == want.counts
    assert got.retracts == want.retracts
    assert sorted(zip(got.redirects, got.redirect_kinds)) == sorted(zip(want.redirects, want.redirect_kinds))
    assert (got.new_free == want.new_free).all()
    assert [int(rec_off[w + 1] - rec_off[w]) for w in range(len(want.records))] == [len(r) for r in want.records]
    return want


@pytest.mark.parametrize("seed", range(150))
def test_host_stages_fuzz_scenarios(seed):
    import test_gpu_fuzz as f
    from oracle.oracle import Oracle

    cfg, envs, _rng = f.build(seed)
    o = Oracle(cfg, canonical=True)
    hs = HostStages(cfg)
    e = envs[1]
    for _ in range(2):
        snap = e.snapshot()
        got = hs.stages(snap)
        if seed < 40:
            _same_mapping_part(hs, snap)
        want = e.schedule(o)
        if not want.is_optimal:
            pytest.skip("oracle hit its limit")
        _same_host_part(got, want, o.last_model())
        done = 0
        for t in sorted(e.tasks.values(), key=lambda t: t.id):
            if t.state == 1 and done < 2:
                e.finish_task(t.id, t.worker); done += 1


@pytest.mark.parametrize("seed", range(300))
def test_host_stages_idle_cluster(seed):
    """few ready tasks on many identical idle workers: the reduced coupled model (empty workers eliminated) against the oracle's full model"""
    import test_gpu_fuzz as f
    from oracle.oracle import Oracle

    cfg, envs = f.build_idle_cluster(20_000 + seed)
    o = Oracle(cfg, canonical=True)
    hs = HostStages(cfg)
    e = envs[1]
    for tick_no in range(2):
        snap = e.snapshot()
        got = hs.stages(snap)
        want = e.schedule(o)
        if not (want.is_optimal and got.is_optimal):
            pytest.skip("a solver hit its limit")
        _same_host_part(got, want, o.last_model())
        for s in range(3):
            e.new_task(TB().cpus(1 + (tick_no + s) % 3))


@pytest.mark.parametrize("name,n_tasks,n_workers", [("c2", 3000, 8), ("c3", 6000, 12), ("c4", 4000, 6), ("c3p", 3000, 6), ("c3", 300, 12), ("c4", 200, 6)])
def test_host_stages_baseline_shapes_reduced(name, n_tasks, n_workers):
    """the BASELINE workload shapes, reduced: saturated (separable path) and unsaturated (lazy size rows / coupled path) sizes"""
    from hyperqueue_amd import workloads
    from oracle.oracle import Oracle

    snap = workloads.make(name, n_workers=n_workers)
    snap.task_id, snap.task_priority, snap.task_rq = snap.task_id[:n_tasks], snap.task_priority[:n_tasks], snap.task_rq[:n_tasks]
    cfg = abi.make_config(time_limit_s=30.0)
    o = Oracle(cfg, canonical=True)
    want = o.tick(snap)
    got = HostStages(cfg).stages(snap)
    if not (want.is_optimal and got.is_optimal):
        pytest.skip("a solver hit its limit")
    _same_host_part(got, want, o.last_model())


def build_unsaturated(seed: int):
    """a handful of workers of one or two kinds, several request shapes over up to three resources, fewer tasks than the cluster holds:
    the coupled model with the batch-size rows binding ("Unsaturated ticks"), at sizes the canonical oracle still solves"""
    from hyperqueue_amd.core import SchedEnv, WorkerBuilder as WB

    rng = np.random.default_rng(seed)
    cfg = abi.make_config(reserve=int(rng.integers(0, 3)), fill_max=int(rng.integers(1, 4)), time_limit_s=30.0)
    e = SchedEnv(cfg)
    names = ["gpus", "mem"][: int(rng.integers(0, 3))]
    for n in names:
        e.new_named_resource(n)
    kinds = []
    for _ in range(int(rng.integers(1, 3))):
        wb = WB(int(rng.integers(8, 33)))
        for n in names:
            wb = wb.res_sum(n, int(rng.integers(2, 9)))
        kinds.append(wb)
    for _ in range(int(rng.integers(3, 9))):
        e.new_worker(kinds[int(rng.integers(0, len(kinds)))])
    shapes = []
    for _ in range(int(rng.integers(2, 6))):
        b = TB().cpus([1, 1, 2, 4, 8][int(rng.integers(0, 5))])
        for ri in range(len(names)):
            if rng.random() < 0.5:
                b = b.add_resource(ri + 1, [0.25, 0.5, 1, 2][int(rng.integers(0, 4))])
        shapes.append(b)
    for _ in range(int(rng.integers(10, 120))):
        e.new_task(shapes[int(rng.integers(0, len(shapes)))])
    return cfg, e


@pytest.mark.parametrize("seed", range(120))
def test_host_stages_unsaturated(seed):
    from oracle.oracle import Oracle

    cfg, e = build_unsaturated(50_000 + seed)
    o = Oracle(cfg, canonical=True)
    snap = e.snapshot()
    got = HostStages(cfg).stages(snap)
    want = o.tick(snap)
    if not (want.is_optimal and got.is_optimal):
        pytest.skip("a solver hit its limit")
    _same_host_part(got, want, o.last_model())


class _QueryOnlyBackend:
    """the reference's query tests call only `query`; anything else here would mean a test that needs the GPU stages"""

    def __init__(self):
        self._hs = {}

    def query(self, snap, *a):
        cfg = getattr(snap, "config", None) or abi.make_config()
        key = (cfg.proactive_filling_reserve, cfg.proactive_filling_max)
        if key not in self._hs:
            self._hs[key] = HostStages(cfg)
        return self._hs[key].query(snap, *a)

    def tick(self, snap):  # a few query tests schedule first: the oracle stands in for the full tick, the query itself goes through the hook
        from oracle.oracle import Oracle

        return Oracle(getattr(snap, "config", None) or abi.make_config(), canonical=True).tick(snap)


def _query_cases():
    import golden_cases

    return [c for c in golden_cases.ALL_CASES if c.__name__.startswith("test_query")]


@pytest.mark.parametrize("case", _query_cases(), ids=lambda f: f.__name__)
def test_reference_query_cases_through_host_hook(case):
    """compute_new_worker_query (tests/test_query.rs, 22 cases) with the host stages of hqtick_query running on this machine"""
    case(_QueryOnlyBackend())


class _ShadowBackend:
    """Every tick of a reference case: the canonical oracle produces the full result the case asserts on; the product's host stages
    (batches + placement through hqtick_debug_host_stages) run on the same snapshot and must give the same batches and counts."""

    def __init__(self):
        self._o, self._hs, self.flags, self.ticks = {}, {}, [], 0

    def _pair(self, snap):
        from oracle.oracle import Oracle

        cfg = getattr(snap, "config", None) or abi.make_config()
        key = (cfg.proactive_filling_reserve, cfg.proactive_filling_max)
        if key not in self._o:
            self._o[key], self._hs[key] = Oracle(cfg, canonical=True), HostStages(cfg)
        return self._o[key], self._hs[key]

    def tick(self, snap):
        o, hs = self._pair(snap)
        want = o.tick(snap)
        got = hs.stages(snap)
        _same_host_part(got, want, o.last_model())
        _same_mapping_part(hs, snap)
        self.flags.append(got.is_canonical == got.is_optimal)
        self.ticks += 1
        return want

    def batches(self, snap):
        o, hs = self._pair(snap)
        want = o.batches(snap)
        assert hs.stages(snap).batches == want
        return want

    def query(self, snap, *a):
        return self._pair(snap)[1].query(snap, *a)


def _tick_cases():
    import golden_cases

    slow = ("test_many_cuts", "test_schedule_many_distinct_shapes_stays_bounded")  # canonicalising 600 / 1200 columns with one HiGHS call each
    return [c for c in golden_cases.ALL_CASES if not c.__name__.startswith("test_query") and c.__name__ not in slow]


@pytest.mark.parametrize("case", _tick_cases(), ids=lambda f: f.__name__)
def test_reference_cases_host_stages_shadow(case):
    """the reference's scheduler tests (sn, mn, batches, end-to-end) on CPU: the product's batches + placement equal the canonical oracle's on
    every tick, and the tie-break phase completes (the assertion tests/test_gpu_golden.py makes on the GPU)"""
    b = _ShadowBackend()
    case(b)
    assert all(b.flags), "tie-break phase cut short on a reference-sized model"


def _extra_cases():
    import golden_cases

    return golden_cases.E2E_EXTRA_CASES


@pytest.mark.parametrize("case", _extra_cases(), ids=lambda f: f.__name__)
def test_e2e_extra_host_stages_shadow(case):
    b = _ShadowBackend()
    case(b)
    assert all(b.flags) and b.ticks >= 1


@pytest.mark.parametrize("seed", range(60))
def test_host_stages_prefill_disposal_family(seed):
    """the scenario family of tests/test_gpu_fuzz.py::test_fuzz_prefill_disposal (priority arrivals dissolving prefill sets, Retracting tasks in the
    queues, retract responses) through the host stages: the coupled models of these ticks have tied optima, so the counts pin the model's COLUMNS
    (the flags the reference creates even for workers without a placement column, solver.rs:233-253) — a round-3 regression the GPU run caught"""
    from hyperqueue_amd.core import SchedEnv, WorkerBuilder as WB
    from oracle.oracle import Oracle

    rng = np.random.default_rng(9000 + seed)
    cfg = abi.make_config(reserve=int(rng.integers(0, 2)), fill_max=int(rng.integers(1, 4)), time_limit_s=20.0)
    e = SchedEnv(cfg)
    o, hs = Oracle(cfg, canonical=True), HostStages(cfg)
    shapes = [TB().cpus(1), TB().cpus(2)]
    for c in [int(x) for x in np.random.default_rng(seed).integers(1, 5, size=3)]:
        e.new_worker(WB(c))
    prio = 0
    for round_ in range(5):
        n_new = int(rng.integers(1, 7)) if round_ else int(rng.integers(8, 16)); which = [int(rng.integers(0, 2)) for _ in range(n_new)]
        if round_ and rng.random() < 0.7:
            prio += 1
        for c in which:
            e.new_task(shapes[c].user_priority(prio))
        snap = e.snapshot()
        _same_mapping_part(hs, snap)
        try:
            want = o.tick(snap)
        except RuntimeError:  # a Retracting task reached the prefill step: the reference asserts there
            return
        got = hs.stages(snap)
        if not (want.is_optimal and got.is_optimal):
            pytest.skip("a solver hit its limit")
        _same_host_part(got, want, o.last_model())
        e.apply(want)
        k = int(rng.integers(1, 7)); answer = rng.random() < 0.6
        done = 0
        for t in sorted(e.tasks.values(), key=lambda t: t.id):
            if t.state == 1 and done < k:
                e.finish_task(t.id, t.worker); done += 1
        if answer:
            for t in [t for t in sorted(e.tasks.values(), key=lambda t: t.id) if t.state == 4 and t.id not in e.retaken_variant][:2]:
                e.retract_response(t.worker, [t.id])


def test_prefill_disposal_family_reaches_every_mapping_outcome():
    """the family above, seeds 0-59 as that test generates them, counted in the oracle's own results: it holds redirects of each of the three kinds, retracts,
    prefill records and ticks on which the reference asserts — so the mapping comparison of that test is one of every outcome of the plan's redirect and
    prefill stages.  (Measured with the oracle alone: 10 FROM_PREFILL, 10 RETARGET, 23 SAME_WORKER redirects, 10 retracts, 235 prefill records, 26 seeds that end
    in the assertion.)"""
    from hyperqueue_amd.core import SchedEnv, WorkerBuilder as WB
    from oracle.oracle import Oracle

    kinds, retracts, prefills, asserted = {abi.HQ_REDIRECT_FROM_PREFILL: 0, abi.HQ_REDIRECT_RETARGET: 0, abi.HQ_REDIRECT_SAME_WORKER: 0}, 0, 0, 0
    for seed in range(60):
        rng = np.random.default_rng(9000 + seed)
        cfg = abi.make_config(reserve=int(rng.integers(0, 2)), fill_max=int(rng.integers(1, 4)), time_limit_s=20.0)
        e = SchedEnv(cfg)
        o = Oracle(cfg, canonical=True)
        shapes = [TB().cpus(1), TB().cpus(2)]
        for c in [int(x) for x in np.random.default_rng(seed).integers(1, 5, size=3)]:
            e.new_worker(WB(c))
        prio = 0
        for round_ in range(5):
            n_new = int(rng.integers(1, 7)) if round_ else int(rng.integers(8, 16)); which = [int(rng.integers(0, 2)) for _ in range(n_new)]
            if round_ and rng.random() < 0.7:
                prio += 1
            for c in which:
                e.new_task(shapes[c].user_priority(prio))
            try:
                want = o.tick(e.snapshot())
            except RuntimeError:
                asserted += 1
                break
            for k in want.redirect_kinds:
                kinds[k] += 1
            retracts += sum(len(r) for r in want.retracts)
            prefills += sum(1 for recs in want.records for (_t, _v, kind) in recs if kind == abi.HQ_REC_PREFILL)
            e.apply(want)
            k = int(rng.integers(1, 7)); answer = rng.random() < 0.6
            done = 0
            for t in sorted(e.tasks.values(), key=lambda t: t.id):
                if t.state == 1 and done < k:
                    e.finish_task(t.id, t.worker); done += 1
            if answer:
                for t in [t for t in sorted(e.tasks.values(), key=lambda t: t.id) if t.state == 4 and t.id not in e.retaken_variant][:2]:
                    e.retract_response(t.worker, [t.id])
    print(kinds, retracts, prefills, asserted)
    assert all(n >= 1 for n in kinds.values()) and retracts >= 1 and prefills >= 1 and asserted >= 1, (kinds, retracts, prefills, asserted)
