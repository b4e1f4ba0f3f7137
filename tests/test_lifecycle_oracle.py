"""The lifecycle histories of tests/lifecycle_cases.py on the SchedEnv mirror alone, every tick taken from the CPU oracle on the mirror's snapshot (SchedEnv.apply
asserts the oracle's new_free against the mirror's own rows): the generator asks only for what the mirror and the reference allow, before any GPU time is spent
on tests/test_gpu_lifecycle.py.  Coverage is a condition HERE: over the seed set of each form every kind of answer and event below occurs in at least two seeds.
Also the zero-selection two-call tick's scenario, built with the oracle.  No GPU needed."""
import collections

import pytest

import lifecycle_cases as lc
from hyperqueue_amd import abi
from oracle.oracle import Oracle

NAMES = {}
for prefix, n in (("HQ_START_", 10), ("HQ_FINISH_", 7), ("HQ_FAIL_", 10), ("HQ_CANCEL_", 6)):
    for name in dir(abi):
        if name.startswith(prefix) and isinstance(getattr(abi, name), int):
            NAMES[f"{prefix}{getattr(abi, name)}"] = name
    assert sum(1 for k in NAMES if k.startswith(prefix)) == n, prefix

REQUIRED = sorted(NAMES) + ["HQ_REDIRECT_FROM_PREFILL", "HQ_REDIRECT_RETARGET", "HQ_REDIRECT_SAME_WORKER", "retract", "PREFILL record", "multi-node placement",
                            "lost worker with a running task", "lost worker with a prefilled task", "lost worker with a Retracting task"]
# what only a tick of two calls can show
TWO_CALL = ["abandoned two-call tick", "two-call tick, zero selected, a redirect"]
# kind -> why no sequence of public calls produces it from this environment.  Expected to be empty; it may hold no accepted kind.
EXEMPT = {}
MIN_SEEDS = 2


@pytest.fixture(scope="module")
def played():
    oracle = Oracle(abi.make_config(reserve=1, fill_max=2, **lc.CFG), canonical=True)
    return {form: [lc.play(lc.history(seed, form), oracle) for seed in lc.SEEDS[form]] for form in lc.FORMS}


def test_seed_counts():
    assert len(lc.SEEDS["two_call"]) >= 12 and len(lc.SEEDS["in_tick"]) >= 12 and len(lc.SEEDS["view"]) >= 4


@pytest.mark.parametrize("form", lc.FORMS)
def test_histories_run_on_the_mirror_and_end_early_only_where_the_reference_refuses(played, form):
    hs = played[form]
    early = [h for h in hs if h.ended_early is not None]
    for h in hs:
        assert 5 <= h.n_rounds <= 8 or h.long
        if h.ended_early is None:
            assert h.rounds_done == h.n_rounds
        else:  # (play() ends a history nowhere else: the oracle's own tick reported a status below zero)
            assert any(k.startswith("tick refused") for k in h.cov) and h.ended_early >= 4, (h.seed, h.ended_early)
    assert len(early) * 4 <= len(hs), [(h.seed, h.ended_early) for h in early]
    assert not any(h.cov["multi-node placement on a worker with prefilled tasks"] for h in hs)  # (out of scope by design, DESIGN.md §8g: the seeds avoid it)
    print(form, "ended early:", [(h.seed, h.ended_early, [k for k in h.cov if k.startswith("tick refused")]) for h in early])


@pytest.mark.parametrize("form", lc.FORMS)
def test_coverage_of_each_form(played, form):
    hs = played[form]
    seeds = collections.defaultdict(set); total = collections.Counter()
    for h in hs:
        for k, n in h.cov.items():
            if n:
                seeds[k].add(h.seed); total[k] += n
    required = REQUIRED + (TWO_CALL if form != "in_tick" else [])
    print(f"\ncoverage, form {form}, {len(hs)} seeds: kind | seeds | occurrences")
    for k in required + sorted(set(seeds) - set(required)):
        print(f"  {NAMES.get(k, k):48s} | {len(seeds[k]):3d} | {total[k]:5d}" + ("   (exempt)" if k in EXEMPT else ""))
    print(f"  ledger entries entered, largest history: {max(h.inserts for h in hs)}")
    accepted = {f"HQ_START_{k}" for k in abi.HQ_START_ACCEPTED} | {f"HQ_FINISH_{k}" for k in abi.HQ_FINISH_ACCEPTED} | {f"HQ_FAIL_{k}" for k in abi.HQ_FAIL_ACCEPTED}
    assert not accepted & set(EXEMPT) and set(EXEMPT) <= set(required)
    missing = {k: len(seeds[k]) for k in required if k not in EXEMPT and len(seeds[k]) < MIN_SEEDS}
    assert not missing, missing


@pytest.mark.parametrize("form", lc.FORMS)
def test_a_history_of_each_form_outgrows_the_ledgers_first_table(played, form):
    """1024 buckets, rebuilt when entries + tombstones pass half of them: the form's long history enters more than 512 entries, in ticks as
    small as every other history's, so claim words and running bytes cross a rebuild between starts, finishes, cancels and lost workers"""
    long = [h for h in played[form] if h.long]
    assert long and all(h.ended_early is None and h.inserts > 512 for h in long), [(h.seed, h.inserts, h.ended_early) for h in long]


def test_the_zero_selection_scenario():
    """the scenario of the regression test (tests/test_gpu_lifecycle.py): the oracle's tick has a redirect and its retract, and no ASSIGN or PREFILL record"""
    cfg = abi.make_config(reserve=1, fill_max=1, **lc.CFG)
    oracle = Oracle(cfg, canonical=True)
    e, w1, w2, assigned, prefilled = lc.zero_selection_env(lambda e, snap: oracle.tick(snap))
    res = oracle.tick(e.snapshot())
    assert len(res.redirects) >= 1 and not any(res.records)
    lc.check_zero_selection_result(e, res, w1, w2, prefilled)
    assert lc.enters_something(e, res)
    e.apply(res)
    assert e.tasks[prefilled].is_retracting() and e.redirects[prefilled] == (w2, 0) and e.workers[w2].free[0] == 0
