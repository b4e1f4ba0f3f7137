"""The grouping of a cancel batch with no HIP in sight (csrc/cancel_core.h): the phase functions of cancel.hip's kernels run on host arrays through
hqtick_debug_cancel_group, in three emulated thread orders, against numpy's stable argsort and bincount; and the stand-alone sanitizer program.  No GPU needed."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperqueue_amd import _testhooks, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
NS = [0, 1, 63, 64, 65, 255, 256, 257, 4097]
WS = [1, 2, 255, 256, 257, 70000]  # one, two and three radix digits


def group(n, W, route, ids, wid, order):
    lib = _testhooks.load()
    f = lib.hqtick_debug_cancel_group
    f.argtypes = [C.c_uint32, C.c_uint32, abi.u32p, abi.u64p, abi.u32p, C.c_int, C.POINTER(C.c_uint32), abi.u32p, abi.u32p, abi.u64p]
    f.restype = C.c_int
    route = np.ascontiguousarray(route, np.uint32); ids = np.ascontiguousarray(ids, np.uint64); wid = np.ascontiguousarray(wid, np.uint32)
    o_w = np.full(W, 0xDEADBEEF, np.uint32); o_off = np.full(W + 1, 0xDEADBEEF, np.uint32); o_id = np.full(n, 0xDEADBEEF, np.uint64)
    nw = C.c_uint32(0xDEADBEEF)
    rc = f(n, W, route.ctypes.data_as(abi.u32p), ids.ctypes.data_as(abi.u64p), wid.ctypes.data_as(abi.u32p), order, C.byref(nw),
           o_w.ctypes.data_as(abi.u32p), o_off.ctypes.data_as(abi.u32p), o_id.ctypes.data_as(abi.u64p))
    assert rc >= 0, rc
    k = nw.value
    assert k <= W and int(o_off[k]) == rc
    return o_w[:k].copy(), o_off[:k + 1].copy(), o_id[:rc].copy()


def expected(W, route, ids, wid):
    """numpy: a stable sort of the routed positions by row, and the rows' counts"""
    route = np.asarray(route, np.uint32)
    pos = np.flatnonzero(route < W)
    order = pos[np.argsort(route[pos], kind="stable")]
    cnt = np.bincount(route[pos].astype(np.int64), minlength=W)
    rows = np.flatnonzero(cnt)
    off = np.concatenate([[0], np.cumsum(cnt[rows])]).astype(np.uint32)
    return np.asarray(wid, np.uint32)[rows], off, np.asarray(ids, np.uint64)[order]


def check(n, W, route, order, rng):
    ids = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    wid = (50 + 3 * np.arange(W)).astype(np.uint32)
    got = group(n, W, route, ids, wid, order)
    exp = expected(W, route, ids, wid)
    for g, e, what in zip(got, exp, ("workers", "offsets", "ids")):
        assert np.array_equal(g, e), (n, W, order, what)


@pytest.mark.parametrize("W", WS)
def test_fixed_routes(W):
    rng = np.random.default_rng(W)
    for n in NS:
        check(n, W, np.full(n, NONE, np.uint32), 0, rng)            # no position routed
        check(n, W, np.full(n, W - 1, np.uint32), 1, rng)           # all on one row (the highest: every digit in use)
        check(n, W, (np.arange(n) % W).astype(np.uint32), 2, rng)   # round-robin over the rows
    check(W, W, rng.permutation(W).astype(np.uint32), 0, rng)        # every row once


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("W", WS)
def test_random_routes_in_three_thread_orders(W, order):
    rng = np.random.default_rng(1000 + W)  # the same inputs in every order
    for n in NS:
        route = rng.integers(0, W, n, dtype=np.uint32)
        drop = rng.random(n) < 0.3
        route[drop] = np.where(rng.random(int(drop.sum())) < 0.5, NONE, W + rng.integers(0, 4, int(drop.sum()))).astype(np.uint32)  # NONE, or anything else not below W
        check(n, W, route, order, rng)


def test_skewed_routes_cross_tiles():
    """one row holding more than a tile of ids between thinly used rows: the per-tile counts of one digit add up across tiles"""
    rng = np.random.default_rng(7)
    n, W = 4097, 300
    route = np.where(rng.random(n) < 0.8, 299, rng.integers(0, W, n)).astype(np.uint32)
    for order in (0, 1, 2):
        check(n, W, route, order, rng)


def test_arguments_are_checked():
    lib = _testhooks.load()
    f = lib.hqtick_debug_cancel_group
    f.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    nw = C.c_uint32(); off = (C.c_uint32 * 2)(); a = (C.c_uint64 * 4)()
    assert f(0, 0, None, None, None, 0, C.byref(nw), None, off, None) == 0 and nw.value == 0 and off[0] == 0
    assert f(0, 0, None, None, None, 3, C.byref(nw), None, off, None) == abi.HQTICK_E_INVALID
    assert f(1, 0, None, a, None, 0, C.byref(nw), None, off, a) == abi.HQTICK_E_INVALID
    assert f(0, 0, None, None, None, 0, None, None, off, None) == abi.HQTICK_E_INVALID


def test_cancel_core_under_sanitizers():
    """tools/cancel_core_asan.cpp: the same phases on batches of 0 .. 4097 positions over 1 .. 70000 rows, every array in an exact-size heap block, under
    AddressSanitizer + UBSan.  A stand-alone program: nothing is loaded into this process."""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "cancel_core_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                               os.path.join(ROOT, "tools", "cancel_core_asan.cpp")])
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "cancel_core_asan:" in p.stdout and "checks" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
