"""Clock mode of the resident worker set (hqtick_cluster_set_clock; csrc/clock_core.h): the canonical remaining lifetime that k_clock_rows writes, run on the CPU
through the debug hook in both of its forms — the linear fold over the request table's thresholds (the kernel's) and the binary search over a sorted copy (the
host mirror's).  No GPU needed."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperqueue_amd import _testhooks, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_LIMIT = abi.HQ_NO_TIME_LIMIT
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
S = 1_000_000_000


def _lib():
    lib = _testhooks.load()
    lib.hqtick_debug_clock_rows.argtypes = [C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    lib.hqtick_debug_clock_deadline.argtypes = [C.c_int64, C.c_int64]; lib.hqtick_debug_clock_deadline.restype = C.c_int64
    lib.hqtick_debug_clock_remaining.argtypes = [C.c_int64, C.c_int64]; lib.hqtick_debug_clock_remaining.restype = C.c_int64
    return lib


def canonical(deadline, now, thr, sorted_form):
    d = np.ascontiguousarray(deadline, np.int64); t = np.ascontiguousarray(thr, np.uint64); out = np.empty(len(d), np.int64)
    assert _lib().hqtick_debug_clock_rows(len(d), d.ctypes.data, int(now), len(t), t.ctypes.data if len(t) else None, int(sorted_form), out.ctypes.data) == 0
    return out


def time_ok(rem: int, min_time: int) -> bool:
    """K2's test (kernels.hip, worker_eval_block; server/worker.rs:320-326)"""
    return rem == NO_LIMIT or (rem >= 0 and rem >= min_time)


def true_remaining(deadline: int, now: int) -> int:
    """deadline - now in exact integers, saturated into the int64 values a finite lifetime can take"""
    return NO_LIMIT if deadline == NO_LIMIT else max(I64_MIN, min(I64_MAX - 1, deadline - now))


def _check(deadlines, now, thr):
    lin, srt = canonical(deadlines, now, thr, 0), canonical(deadlines, now, thr, 1)
    assert (lin == srt).all()
    passes = {}
    for d, c in zip([int(x) for x in deadlines], lin.tolist()):
        r = true_remaining(d, now)
        subset = tuple(time_ok(r, int(t)) for t in thr) + (r == NO_LIMIT, r >= 0)
        assert tuple(time_ok(c, int(t)) for t in thr) + (c == NO_LIMIT, c >= 0) == subset, (d, now, c)
        assert (c == NO_LIMIT) == (d == NO_LIMIT)
        assert passes.setdefault(subset, c) == c, "workers that pass the same thresholds must get the same value"
    return lin


@pytest.mark.parametrize("seed", range(20))
def test_canonical_value_answers_every_threshold_like_the_true_lifetime(seed):
    rng = np.random.default_rng(seed)
    nv = int(rng.integers(0, 12)) if seed % 5 else 600  # (600: more than two of the kernel's chunks)
    thr = (rng.integers(0, 200, size=nv) * S).astype(np.uint64)
    thr[rng.random(nv) < 0.2] = 0
    now = int(rng.integers(-100 * S, 300 * S))
    d = now + rng.integers(-50 * S, 250 * S, size=400)
    d[rng.random(400) < 0.1] = NO_LIMIT
    if nv:  # some deadlines exactly on a threshold and one below
        d[:20] = now + rng.choice(thr, 20).astype(np.int64) - rng.integers(0, 2, size=20)
    _check(d, now, thr)


def test_edges():
    thr = [0, 10 * S, 100 * S, 10 * S]  # a duplicate
    now = 7 * S
    assert _check([NO_LIMIT], now, thr).tolist() == [NO_LIMIT]
    assert _check([now - 1, I64_MIN], now, thr).tolist() == [-1, -1]                        # past the deadline
    assert _check([now], now, thr).tolist() == [0]                                          # deadline == now: a zero min_time passes ...
    assert time_ok(0, 0) and not time_ok(0, 1) and _check([now], now, [1, 5]).tolist() == [0]  # ... anything else does not
    assert _check([now + 10 * S, now + 10 * S - 1, now + 100 * S, now + 100 * S - 1], now, thr).tolist() == [10 * S, 0, 100 * S, 10 * S]
    assert _check([now + 5, now - 5, NO_LIMIT], now, []).tolist() == [0, -1, NO_LIMIT]        # nv == 0
    big = [0, 1 << 63, (1 << 64) - 1, 5 * S]                                                # thresholds no int64 lifetime reaches
    assert _check([now + 6 * S, I64_MAX - 1], now, big).tolist() == [5 * S, 5 * S]
    assert _check([I64_MAX - 1], -5, [I64_MAX - 1, I64_MAX]).tolist() == [I64_MAX - 1]      # the difference saturates below HQ_NO_TIME_LIMIT
    # both ends of the int64 range
    for d in (I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, NO_LIMIT):
        for n in (I64_MIN, -1, 0, 1, I64_MAX):
            _check([d], n, thr); _check([d], n, big)


def test_deadline_and_remaining_saturate():
    lib = _lib()
    dl, rm = lib.hqtick_debug_clock_deadline, lib.hqtick_debug_clock_remaining
    assert dl(5, NO_LIMIT) == NO_LIMIT and dl(I64_MIN, NO_LIMIT) == NO_LIMIT
    assert dl(100, 50) == 150 and dl(-100, 50) == -50 and dl(100, -50) == 50
    assert dl(I64_MAX, 1) == I64_MAX - 1 and dl(I64_MAX, I64_MAX - 1) == I64_MAX - 1 and dl(1, I64_MAX - 1) == I64_MAX - 1  # never becomes "no limit"
    assert dl(I64_MIN, -1) == I64_MIN and dl(I64_MIN, I64_MIN) == I64_MIN
    assert rm(NO_LIMIT, 123) == NO_LIMIT
    assert rm(I64_MAX - 1, I64_MIN) == I64_MAX - 1 and rm(I64_MAX - 1, -1) == I64_MAX - 1 and rm(I64_MIN, I64_MAX) == I64_MIN and rm(I64_MIN, 1) == I64_MIN
    for d, n in ((0, 0), (10, 3), (3, 10), (-5, -9), (I64_MAX - 1, I64_MAX), (I64_MIN, I64_MIN)):
        assert rm(d, n) == true_remaining(d, n)
    # a host that uploaded lifetimes taken at `now` loses nothing
    for now in (0, -3 * S, 1 << 40):
        for rem in (0, 1, -1, 17 * S, NO_LIMIT):
            assert rm(dl(now, rem), now) == rem


def test_phase_function_under_sanitizers():
    """tools/clock_core_asan.cpp: the phase function over the edge cases and a random campaign under AddressSanitizer + UBSan, every table in an exact-size heap
    block.  A stand-alone program: nothing is loaded into this process."""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "clock_core_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "clock_core_asan.cpp")])
        p = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "checks ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_host_stages_take_canonical_lifetimes_like_true_ones():
    """the tick's host stages (batches, placement) on K2's answers: the same batches and counts for the canonical lifetimes as for the true ones — and the canonical
    ones leave far fewer groups of equal rows to work on"""
    import dataclasses

    from hyperqueue_amd import workloads
    from host_stages import HostStages

    def variant(entries, min_time_s):
        v = workloads._variant(entries); v["min_time_ns"] = min_time_s * S
        return v

    reqs = [[variant([(0, 1)], 0)], [variant([(0, 4)], 10)], [variant([(0, 2), (1, 1)], 100)], [variant([(0, 8)], 100), variant([(0, 2)], 10)]]
    W, n = 40, 4_000
    total = np.tile(np.asarray([16, 2], np.uint64) * np.uint64(workloads.FR), (W, 1))
    term = (np.arange(W, dtype=np.int64) * 5 - 20) * S + np.arange(W, dtype=np.int64) * 1017
    term[::7] = NO_LIMIT
    ids = (np.uint64(1) << np.uint64(32)) | np.arange(1, n + 1, dtype=np.uint64)
    h = HostStages(abi.make_config(time_limit_s=20.0))
    thr = [v["min_time_ns"] for r in reqs for v in r]
    for now in (0, 33 * S, 131 * S):
        rem = np.where(term == NO_LIMIT, NO_LIMIT, term - now).astype(np.int64)
        snap = abi.Snapshot(n_resources=2, worker_id=np.arange(1, W + 1, dtype=np.uint32), worker_total=total, worker_free=total.copy(), worker_remaining_ns=rem,
                            worker_min_utilization=np.zeros(W, np.float32), worker_flags=np.full(W, abi.HQ_WORKER_SN, np.uint8), worker_group=np.zeros(W, np.uint32), n_groups=1,
                            blocked=[], assigned=[[] for _ in range(W)], prefilled=[[] for _ in range(W)], requests=reqs, task_id=ids,
                            task_priority=np.full(n, workloads.priority_from_user(0), np.uint64), task_rq=(np.arange(n) % 4).astype(np.uint32))
        can = canonical(term, now, thr, 1)
        assert len(set(can.tolist())) <= 5 < len(set(rem.tolist()))
        a, b = h.stages(snap), h.stages(dataclasses.replace(snap, _keep=[], worker_remaining_ns=can))
        assert a.status == b.status and a.batches == b.batches and a.counts == b.counts and len(a.counts) > 0
