"""The resident attribute table of the wire encoder (hqwire_table_*, include/hqwire.h) on a real MI355X: the table in HBM, its deltas as kernels, and
hqwire_encode_device reading it through hqwire_table_view.  Byte for byte against the bincode oracle, WireTables.build and the host debug backend.
(Sorts behind test_zz_gpu_wire.py: the encoder's own tests come first.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import wire_cases as wc
import wire_table_cases as tc
from hyperqueue_amd import wire

pytestmark = pytest.mark.gpu
TILE = tc.TILE
SMALL = dict(initial_rows=8, initial_blob_bytes=64, initial_configs=1, initial_body_bytes=8)


def device_table(**kw):
    return wire.WireTable(**kw)


def encode(t, r, cap):
    return wire.encode_device(t, r, cap)


@pytest.fixture(scope="module")
def table_canary():
    """First contact of the table's kernels with hardware happens in a SUBPROCESS: a device fault there ends that process, not the GPU suite.  Every
    test of this module depends on it; nothing is retried."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch  # (its HIP runtime first, as in conftest.py)\n"
            "import wire_table_cases as tc\nfrom hyperqueue_amd import wire\n"
            "t = wire.WireTable()\ntc.run_sequence(0, t, wire.encode_device, n_ops=10)\nt.close()\n"
            "tc.tile_boundary_case(wire.WireTable, wire.encode_device, tc.TILE + 1)\nprint('canary ok')\n") % (os.path.join(here, ".."), here)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    if p.returncode != 0 or "canary ok" not in p.stdout:
        pytest.fail("the table's kernels failed their first hardware run (subprocess): exit %s\n%s" % (p.returncode, (p.stdout + p.stderr)[-2500:]))
    return True


@pytest.mark.parametrize("seed", range(6))
def test_device_delta_sequences(seed, table_canary):
    """six of the CPU suite's sequences (odd seeds from tiny allocations: every growth path), at most three tiles of rows: after every op an encode on the
    view against the oracle, after every compaction copy_out against WireTables.build"""
    t = device_table(**(SMALL if seed % 2 else {}))
    tc.run_sequence(seed, t, encode)
    t.close()


@pytest.mark.parametrize("rows", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_device_tile_boundaries(rows, table_canary):
    tc.tile_boundary_case(device_table, encode, rows)


def test_device_entry_sizes_at_every_alignment(table_canary):
    tc.entry_sizes_case(device_table, encode)


@pytest.mark.parametrize("seed", [3, 4])
def test_device_and_host_backends_agree(seed, table_canary):
    """copy_out and the stats counters of the device table and of the host table after every op of one sequence"""
    trails = []
    for make, enc in ((lambda: device_table(**SMALL), encode), (lambda: wire.WireTable(host_order=0, **SMALL), lambda t, r, cap: wire.encode_host_debug(t, r, cap))):
        trail, t = [], make()
        tc.run_sequence(seed, t, enc, after_op=lambda t, m: trail.append((tc.digest(t.copy_out()), sorted(t.counters().items()))))
        t.close()
        trails.append(trail)
    assert trails[0] == trails[1] and len(trails[0]) >= 10


def test_device_refusal_and_counts(table_canary):
    t, a = tc.fresh(device_table, [10, 20, 30, 50], lambda i, t: b"ab" * i)
    assert t.remove_tasks([30, 30, 99]) == 1 and t.last_unknown() == 2
    before = tc.digest(t.copy_out())
    for bad in ({20: (0, 0, 0, 0, None)}, {60: (0, 0, 0, 2, None)}):  # a live id (merge path); a configuration index (append path)
        with pytest.raises(Exception):
            t.add_tasks(bad)
        assert tc.digest(t.copy_out()) == before
    assert t.set_instance([10, 10, 30]) == 2 and t.last_unknown() == 1
    assert t.add_tasks({30: (1, 1, 1, 1, b"back")}) == 1
    a[10] = a[10][:1] + (a[10][1] + 2,) + a[10][2:]
    a[30] = (1, 1, 1, 1, b"back")
    tc.assert_equals_build(t, a, tc.CFG)
    assert t.stats().last_kernel_us > 0 and t.stats().hbm_bytes > 0
    t.close()


def test_encode_on_a_table_uploads_no_table(table_canary):
    """encode_device with a WireTable copies the tick's records to the device and nothing else"""
    t, a = tc.fresh(device_table, [(1 << 32) | i for i in range(1, 600)], lambda i, t: b"e" * (i % 9))
    r = wire.WireRecords.build([7, 8], [[(x, 0, 1) for x in sorted(a)[:300]], [(x, 0xFF, 0) for x in sorted(a)[300:]]], [[], []], [])
    rec_bytes = sum(wire._padded(x).nbytes for x in r.arrays())
    before = wire.uploaded_bytes
    res = wire.encode_device(t, r, 1 << 20)
    assert wire.uploaded_bytes - before == rec_bytes
    tables = wire.WireTables.build(a, tc.CFG)
    before = wire.uploaded_bytes
    ref = wire.encode_device(tables, r, 1 << 20)
    assert wire.uploaded_bytes - before == rec_bytes + sum(wire._padded(x).nbytes for x in tables.arrays()) > 37 * len(a)
    assert res.data == ref.data and res.messages(r) == wc.oracle_messages(a, tc.CFG, [7, 8], [[(x, 0, 1) for x in sorted(a)[:300]], [(x, 0xFF, 0) for x in sorted(a)[300:]]], [[], []], [])
    t.close()


def test_chained_ticks_to_bytes(table_canary):
    """tick -> ledger -> bytes over three ticks with ONE resident table (modelled on test_gpu_assigned_forms.py::test_tick_to_bytes_with_the_ledger_on):
    resident workers, the ledger and a record sink on; the records never leave HBM, the table is fed by deltas and never uploaded"""
    from hyperqueue_amd.sharded import sink_layout
    from hyperqueue_amd.tick import Tick
    from test_gpu_assigned_forms import Sink, _ledger_tick

    table = device_table()
    cap = 4096

    class Driver:
        a, sink = None, None

        def tick(self, snap, want):
            W = len(snap.worker_id)
            if self.a is None:
                from hyperqueue_amd import abi

                self.a = Tick(abi.make_config(time_limit_s=20.0))
                self.a.cluster_upload(snap)
                self.a.assigned_enable([])
                self.sink = Sink(self.a, sink_layout(W, cap)[4])
            got = _ledger_tick(self.a, snap, self.sink)
            assert got.records == want.records and got.retracts == want.retracts
            assert self.a.assigned_last_host_bytes() == 0
            n_records = sum(len(r) for r in got.records)
            side = wire.WireRecords.build([int(w) for w in snap.worker_id], want.records, want.retracts, [])
            before = wire.uploaded_bytes
            res = wire.encode_from_sink(table, self.sink.buf, W, 0, n_records, side, 1 << 22)
            assert wire.uploaded_bytes - before == sum(wire._padded(x).nbytes for x in side.arrays())  # the side arrays; no table
            return res

        def release(self, ids):
            assert self.a.assigned_release(ids) == len(ids)

        def lose(self, wid, back):
            assert self.a.cluster_remove_workers([wid]) == []
            return [t for (t, _, _) in self.a.cluster_last_requeued()]

    d = Driver()
    try:
        attrs, configs = tc.chained_ticks(table, d)
        assert table.counters()["appends"] == 3
    finally:
        if d.a is not None:
            d.a.close()
        table.close()
