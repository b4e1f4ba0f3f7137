"""The resident attribute table of the wire encoder (include/hqwire.h, hqwire_table_*) on a machine without a GPU: the very class and kernel phases of
the device path (csrc/wire_table_core.h) on the host debug backend, in all three emulated thread orders, mirrored in a Python dict.  Everything is compared
byte for byte: encodes on the view against the bincode oracle for the dict, copy_out after a compaction against WireTables.build."""
import ctypes as C
import os
import random
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import wire_cases as wc
import wire_table_cases as tc
from hyperqueue_amd import tick, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = tc.TILE
ORDERS = (0, 1, 2)
CFG = tc.CFG


def host_table(order=0, **kw):
    return wire.WireTable(host_order=order, **kw)


def encode(order):
    return lambda t, r, cap: wire.encode_host_debug(t, r, cap, order)


def fresh(order, ids, entry=lambda i, t: None, **kw):
    return tc.fresh(lambda **k: host_table(order, **k), ids, entry, **kw)


attrs_of = tc.attrs_of


@pytest.mark.parametrize("seed", range(20))
def test_random_delta_sequences(seed):
    """append and merge adds (ids below, between and equal to dead ids), removes, instance increments and assignments, add_configs, forced and automatic
    compaction; the three thread orders must leave the same arrays and counters after every op"""
    trails = []
    for order in ORDERS:
        trail = []
        small = dict(initial_rows=8, initial_blob_bytes=64, initial_configs=1, initial_body_bytes=8) if seed % 2 else {}
        table = host_table(order, **small)
        tc.run_sequence(seed, table, encode(order), after_op=lambda t, m: trail.append((tc.digest(t.copy_out()), sorted(t.counters().items()))))
        trails.append(trail)
        table.close()
    assert trails[0] == trails[1] == trails[2] and len(trails[0]) >= 10


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("rows", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_tile_boundaries(rows, order):
    tc.tile_boundary_case(lambda **k: host_table(order, **k), encode(order), rows)


@pytest.mark.parametrize("order", ORDERS)
def test_everything_removed(order):
    ids = [(1 << 32) | i for i in range(1, TILE + 6)]
    t, a = fresh(order, ids, lambda i, t: b"x" * (i % 5))
    assert t.remove_tasks(ids) == len(ids)  # more dead than live: compacts by itself
    st = t.counters()
    assert st["live_rows"] == st["physical_rows"] == st["blob_bytes"] == 0 and st["compactions"] == 1
    assert t.view().n_tasks == 0
    r = wire.WireRecords.build([4, 5], [[], []], [[], [9]], [])
    res = wire.encode_host_debug(t, r, 64, order)
    assert res.status == wire.HQWIRE_OK and len(res.messages(r)) == 1  # an empty tick (one retract list) still encodes
    tc.assert_equals_build(t, {}, CFG)
    b = attrs_of([5, 6, 7])  # ids below the old ones: the table holds nothing, so this is an append
    assert t.add_tasks(b) == 3 and t.counters()["appends"] == 2
    tc.assert_equals_build(t, b, CFG)


@pytest.mark.parametrize("order", ORDERS)
def test_entry_sizes_at_every_alignment(order):
    tc.entry_sizes_case(lambda **k: host_table(order, **k), encode(order))


@pytest.mark.parametrize("order", ORDERS)
def test_chained_ticks_on_the_host_backend(order):
    """the three-tick scenario of the GPU suite (new tasks, finished tasks, a lost worker's tasks requeued with a raised instance id) with the oracle's
    mapping encoded by the emulated phases"""
    table = host_table(order)

    class Driver:
        def tick(self, snap, want):
            return wire.encode_host_debug(table, wire.WireRecords.build([int(w) for w in snap.worker_id], want.records, want.retracts, []), 1 << 22, order)

        def release(self, ids):
            pass

        def lose(self, wid, back):
            return back

    attrs, configs = tc.chained_ticks(table, Driver())
    table.compact()
    tc.assert_equals_build(table, attrs, configs)


def _refusals():
    ok = dict(task_id=[100, 101, 102], task_rq=[1, 2, 3], task_instance=[0, 0, 0], task_priority=[5, 5, 5], task_config=[0, 1, 0],
              entry_some=[1, 0, 1], entry_off=[0, 2, 2, 3], entry_blob=[7, 8, 9])
    yield "ids not ascending", dict(ok, task_id=[100, 102, 101])
    yield "ids equal", dict(ok, task_id=[100, 100, 101])
    yield "id of a live row (append)", dict(ok, task_id=[50, 101, 102])
    yield "id of a live row (merge)", dict(ok, task_id=[10, 20, 21])
    yield "not ascending (merge)", dict(ok, task_id=[11, 9, 12])
    yield "configuration index", dict(ok, task_config=[0, 2, 0])
    yield "entry_off not monotone", dict(ok, entry_off=[0, 3, 2, 3])
    yield "entry_off ends below its start", dict(ok, entry_off=[5, 2, 2, 3])
    yield "None with a length", dict(ok, entry_some=[1, 0, 0])
    yield "reserved id", dict(ok, task_id=[100, 101, 0xFFFFFFFFFFFFFFFE])
    yield "reserved id (merge)", dict(ok, task_id=[11, 12, 0xFFFFFFFFFFFFFFFF])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", list(_refusals()), ids=lambda c: c[0])
def test_refused_batches_change_nothing(case, order):
    t, a = fresh(order, [10, 20, 30, 50], lambda i, t: b"ab" * i)
    assert t.remove_tasks([30]) == 1  # (a dead row in the table: a refused merge must not even drop it)
    before, counters = tc.digest(t.copy_out()), t.counters()
    with pytest.raises(tick.HqTickError) as e:
        t.add_tasks_arrays(**case[1])
    assert e.value.code == -1 and ("refused" in str(e.value) or "monotone" in str(e.value))
    assert tc.digest(t.copy_out()) == before and t.counters() == counters
    good = {30: (1, 1, 1, 1, b"back"), 31: (0, 0, 0, 0, None)}  # the next valid add succeeds (a merge that brings a dead id back)
    assert t.add_tasks(good) == 2
    del a[30]
    a.update(good)
    tc.assert_equals_build(t, a, CFG)


def test_row_total_limit():
    t, a = fresh(0, [1, 2, 3])
    before = tc.digest(t.copy_out())
    lib = t.lib
    one = np.zeros(1, np.uint64)
    # n alone reaches the limit: refused before any array is read
    assert lib.hqwire_table_add_tasks(t.h, 0xFFFFFFFF, one.ctypes.data, one.ctypes.data, None, one.ctypes.data, one.ctypes.data, None, None, None) == -1
    assert lib.hqwire_table_add_tasks(t.h, 0xFFFFFFFF - 3, one.ctypes.data, one.ctypes.data, None, one.ctypes.data, one.ctypes.data, None, None, None) == -1  # with the 3 resident rows
    assert "0xFFFFFFFF" in t.last_error() and tc.digest(t.copy_out()) == before
    assert t.add_tasks({5: (0, 0, 0, 0, None)}) == 1


@pytest.mark.parametrize("order", ORDERS)
def test_empty_calls_change_nothing(order):
    t, a = fresh(order, [10, 20, 30])
    before, counters = tc.digest(t.copy_out()), t.counters()
    assert t.add_tasks({}) == 0 and t.remove_tasks([]) == 0 and t.set_instance([]) == 0 and t.set_instance([], []) == 0
    assert t.add_configs([]) == len(CFG)
    t.compact()
    assert tc.digest(t.copy_out()) == before and t.counters() == counters


@pytest.mark.parametrize("order", ORDERS)
def test_counts(order):
    t, a = fresh(order, [10, 20, 30, 40, 50])
    assert t.remove_tasks([20, 99, 20, 20]) == 1 and t.last_unknown() == 3       # unknown and repeated ids
    assert t.remove_tasks([20, 10]) == 1 and t.last_unknown() == 1               # already removed
    assert t.set_instance([30, 30, 20, 77, 40]) == 3 and t.last_unknown() == 2   # dead and unknown ids
    assert t.set_instance([50, 10], [9, 9]) == 1 and t.last_unknown() == 1
    t.compact()
    got = t.copy_out()
    assert got.task_id.tolist() == [30, 40, 50] and got.task_instance.tolist() == [2 + 2, 3 + 1, 9]  # listed twice: risen by two
    assert t.remove_tasks([10, 20]) == 0 and t.last_unknown() == 2               # compacted away: unknown now


@pytest.mark.parametrize("order", ORDERS)
def test_growth(order):
    t = host_table(order, initial_rows=4, initial_blob_bytes=16, initial_configs=1, initial_body_bytes=4)
    cfgs = [(None, b"0123456789"), ((1, 2), b"abc"), (None, b"")]
    assert t.add_configs(cfgs[:1]) == 0 and t.add_configs(cfgs[1:]) == 1
    rnd, a, nxt = random.Random(5), {}, (1 << 32) | 1
    for _ in range(143):  # 1001 rows in batches of 7
        batch = {nxt + k: tc.rand_attr(rnd, 3) for k in range(7)}
        nxt += 7
        assert t.add_tasks(batch) == 7
        a.update(batch)
    st = t.counters()
    assert st["live_rows"] == st["physical_rows"] == 1001 and st["appends"] == 143 and st["growths"] >= 9 and st["compactions"] == 0
    tc.assert_equals_build(t, a, cfgs)
    tc.check_encode(rnd, encode(order), t, a, cfgs)


@pytest.mark.parametrize("order", ORDERS)
def test_automatic_compaction_thresholds(order):
    ids = list(range(100, 120))
    t, a = fresh(order, ids, lambda i, t: b"e" * 10 if i >= 18 else None)  # 20 rows, 20 blob bytes on the last two
    assert t.remove_tasks(ids[:10]) == 10 and t.counters()["compactions"] == 0       # 10 dead, 10 live: not MORE dead than live
    assert t.remove_tasks(ids[10:11]) == 1                                          # 11 dead, 9 live
    st = t.counters()
    assert st["compactions"] == 1 and st["physical_rows"] == 9 and st["dead_blob_bytes"] == 0
    assert t.remove_tasks([ids[18]]) == 1                                           # 1 dead of 9 rows, but 10 dead bytes = 10 live bytes
    assert t.counters()["compactions"] == 1 and t.counters()["dead_blob_bytes"] == 10
    b = {200: (0, 0, 0, 0, b"zz")}
    assert t.add_tasks(b) == 1 and t.counters()["compactions"] == 1                 # 10 dead bytes, 12 live
    assert t.remove_tasks([200]) == 1                                               # 12 dead bytes > 10 live: the byte threshold
    st = t.counters()
    assert st["compactions"] == 2 and st["physical_rows"] == 8 and st["blob_bytes"] == 10
    tc.assert_equals_build(t, {i: v for i, v in a.items() if i in ids[11:18] + ids[19:]}, CFG)


def test_abi_version_and_struct_layouts():
    lib = wire.load()
    assert lib.hqwire_abi_version() == wire.HQWIRE_ABI_VERSION == 3
    pairs = {"hqwire_table_config": wire.TableConfigC, "hqwire_table_stats": wire.TableStatsC}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "hqwire.h"', "int main(void){", 'printf("tile %u\\n", HQWIRE_TABLE_TILE);']
    for cname, cls in pairs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = dict(l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l)
    assert int(got["tile"]) == wire.HQWIRE_TABLE_TILE
    for cname, cls in pairs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"


def test_no_cpu_path_in_the_product():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the no-device path cannot be observed")
    with pytest.raises(tick.HqTickError) as e:
        wire.WireTable()
    assert e.value.code == -2  # HQTICK_E_NO_DEVICE
    assert not hasattr(wire.load(), "hqwire_debug_table_create_host")


def test_table_under_sanitizers():
    """tools/wire_table_asan.py: random delta sequences on the host backend under AddressSanitizer + UBSan, a stand-alone program (nothing is loaded
    into python), every allocation an exact-size heap block and the tables sized so that the last append fills them to the byte"""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "HQTICK_TEST_LIB")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "wire_table_asan.py"), "--seeds", "6"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "0 problems" in p.stdout
