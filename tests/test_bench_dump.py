"""bench.py --dump-outputs: the arrays it writes hold the tick's result exactly (float64, task ids split into job / task in job), stay under the
size limit by a fixed row sample, and are the same from run to run.  Fed with a CPU oracle tick here; on the GPU box bench.py feeds it the timed tick."""
import os

import numpy as np

import bench
from hyperqueue_amd import abi, workloads
from oracle.oracle import Oracle


def _tick():
    snap = workloads.make("c3", seed=0, n_tasks=20_000, n_workers=64)
    return snap, Oracle(abi.make_config(time_limit_s=5.0)).tick(snap)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_holds_the_result(tmp_path):
    snap, r = _tick()
    shapes = bench.dump_outputs(str(tmp_path), r)
    got = _load(tmp_path)
    assert set(got) == set(shapes) and all(a.dtype == np.float64 and a.size > 0 for a in got.values())
    assert not ({"retracts", "redirects", "multi_node"} & set(got))  # a cold tick has none: no empty files
    rec = got["records"]
    want = [(w, t, v, k) for w, recs in enumerate(r.records) for (t, v, k) in recs]
    assert len(want) > 0 and rec.shape == (len(want), 5)
    ids = (rec[:, 1].astype(np.uint64) << np.uint64(32)) | rec[:, 2].astype(np.uint64)
    assert ids.tolist() == [x[1] for x in want]
    assert rec[:, 0].astype(int).tolist() == [x[0] for x in want] and rec[:, 3:].astype(int).tolist() == [[x[2], x[3]] for x in want]
    assert got["counts"].astype(int).tolist() == [list(c) for c in r.counts]
    assert (got["new_free"] == r.new_free).all() and got["new_free"].shape == (len(snap.worker_id), snap.n_resources)
    assert got["batches"][:, 0].astype(int).tolist() == [b.rq for b in r.batches]
    assert got["status"].tolist() == [r.status, r.is_optimal, r.is_canonical]


def test_dump_is_capped_and_repeatable(tmp_path, monkeypatch):
    _, r = _tick()
    full = tmp_path / "full"
    bench.dump_outputs(str(full), r)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 200_000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), r)
    bench.dump_outputs(str(b), r)
    ga, gb, gf = _load(a), _load(b), _load(full)
    assert sum(x.nbytes for x in ga.values()) <= 200_000
    assert set(ga) == set(gb) and all(np.array_equal(ga[k], gb[k]) for k in ga)
    rows = ga["records_rows"].astype(np.int64)
    assert 0 < len(rows) < len(gf["records"]) and (np.diff(rows) > 0).all()
    assert np.array_equal(ga["records"], gf["records"][rows])
