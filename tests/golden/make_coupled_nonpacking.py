#!/usr/bin/env python
"""Pinned reference answers of the non-packing coupled family (tests/coupled_cases.py), written to nonpacking/coupled_nonpacking.json.  Run from the repo root:
python tests/golden/make_coupled_nonpacking.py [procs]

Each case is solved by the EXACT oracle, Oracle(make_config(time_limit_s=60)): HiGHS with mip_rel_gap = 0, once with and once without presolve, the better
point that satisfies every row kept (oracle/oracle.py _highs).  Stored per case: that best verified objective, whether a run proved it optimal, the model's
column and row counts and a digest of its objective and rows (coupled_cases.model_digest).  The tests rebuild the model and fail on a digest that no longer
matches: a pin is never compared against another model.  The GPU suite reads the pins and runs no HiGHS.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "nonpacking", "coupled_nonpacking.json")
TIME_LIMIT_S = 60.0


def pin(vs):
    import numpy as np

    import coupled_cases as cc
    from hyperqueue_amd import abi
    from oracle.oracle import Oracle

    variant, seed = vs
    snap = cc.case(variant, seed)
    built = cc.case_model(variant, snap)
    o = Oracle(abi.make_config(time_limit_s=TIME_LIMIT_S))
    t0 = time.time()
    r = o.tick(snap)
    dt = time.time() - t0
    m = o.last_model()
    assert cc.model_digest(m) == cc.model_digest(built), "the solved model is not the one the tests rebuild"
    z = float(np.dot(m["obj"], m["x"]))
    assert abs(z - float(m["objective"])) <= 1e-9 * max(1.0, abs(z))
    return f"{variant}/{seed}", dict(objective=z, proved_optimal=bool(r.is_optimal), cols=len(m["obj"]), rows=len(m["rhs"]), digest=cc.model_digest(m),
                                     solve_s=round(dt, 1))


def main():
    from multiprocessing import Pool

    import coupled_cases as cc

    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    keys = [(v, s) for v in cc.VARIANTS for s in cc.SEEDS[v]]
    with Pool(procs) as p:
        got = dict(p.map(pin, keys, chunksize=1))
    with open(OUT, "w") as f:
        json.dump(dict(oracle=f"Oracle(make_config(time_limit_s={TIME_LIMIT_S:g})): exact HiGHS, presolve off and on, best verified point",
                       cases={k: got[k] for k in sorted(got)}), f, indent=1, sort_keys=True)
    print(f"{len(got)} cases written, {sum(c['proved_optimal'] for c in got.values())} proved optimal")


if __name__ == "__main__":
    main()
