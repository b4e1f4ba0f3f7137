"""hqtick_resident_check's invariants (csrc/audit_core.h) on host arrays, without a GPU: the item functions the kernels of csrc/audit.hip run, executed through
hqtick_debug_audit_host in three emulated thread orders, against the plain restatement of every invariant in tests/audit_cases.py."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import audit_cases as ac
from hyperqueue_amd import _testhooks, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(st, parts, order):
    lib = _testhooks.load()
    lib.hqtick_debug_audit_host.argtypes = [C.POINTER(ac.AuditTablesC), C.c_uint32, C.c_int, C.POINTER(abi.CheckReportC)]
    c, keep = ac.to_c(st)
    r = abi.CheckReportC()
    rc = lib.hqtick_debug_audit_host(C.byref(c), parts, order, C.byref(r))
    d = abi.parse_check_report(r)
    assert rc == d["n_failed"]
    del keep
    return d


def _three_orders(st, parts):
    reps = [_host(st, parts, o) for o in (0, 1, 2)]
    assert reps[0] == reps[1] == reps[2], "the report depends on the order of the emulated threads"
    return reps[0]


@pytest.fixture(scope="module")
def clean():
    return ac.consistent()


def test_consistent_state_is_clean_in_every_order(clean):
    for parts in (abi.HQ_CHECK_ALL, ac.STRICT_ALL):
        rep = _three_orders(clean, parts)
        assert rep["failed"] == {} and rep["n_failed"] == 0
        assert rep["checked"] == parts
        assert all(v == ac.M64 for v in rep["first"].values())
        assert ac.expect(clean, parts) == (parts, {})
    # what makes the state worth auditing: wide count rows, a probe that wraps, a run longer than a wavefront, stale edges, rows at and past 256
    assert clean["l_stride"] == 32 and clean["ready_n"] == 300 and max(clean["g_run_len"]) == 70
    assert ac.ht_find(clean["l_key"], 63, clean["_names"]["wrap"][1]) == 0


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_one_corruption_fires_its_invariant_and_what_it_implies(name):
    _, parts, about, implied = ac.CASES[name]
    st = ac.corrupted(name)
    checked, want = ac.expect(st, parts)
    assert set(want) == {about, *implied}, f"the restatement finds {sorted(want)}"
    rep = _three_orders(st, parts)
    assert rep["checked"] == checked == parts
    assert rep["failed"] == want
    assert rep["n_failed"] == len(want)
    for n in abi.HQ_INV_NAMES:
        if n not in want:
            assert rep["count"][n] == 0 and rep["first"][n] == ac.M64, n


def test_witnesses_of_the_cases_the_issue_names():
    """the exact keys: position 256 and the last row of the ready column, the key cut off behind the last bucket, the consumer behind edge 69, the saturated product"""
    clean = ac.consistent()
    rep = _three_orders(ac.corrupted("ready_order_256"), abi.HQ_CHECK_ALL)
    assert rep["failed"] == {"HQ_INV_READY_ORDER": (1, int(clean["ready_id"][255]))}
    rep = _three_orders(ac.corrupted("ready_order_last"), abi.HQ_CHECK_ALL)
    assert rep["failed"] == {"HQ_INV_READY_ORDER": (1, 0)}
    rep = _three_orders(ac.corrupted("ledger_hash_wrap"), abi.HQ_CHECK_ALL)
    assert rep["failed"]["HQ_INV_LEDGER_HASH"] == (1, clean["_names"]["wrap"][1])
    assert rep["failed"]["HQ_INV_LEDGER_COUNTS"] == (1, 8 << 32 | 0)
    rep = _three_orders(ac.corrupted("graph_counter_fan"), abi.HQ_CHECK_ALL)
    assert rep["failed"] == {"HQ_INV_GRAPH_COUNTER": (1, 668)}
    rep = _three_orders(ac.corrupted("ledger_free_wrapped"), abi.HQ_CHECK_ALL)
    assert rep["failed"] == {"HQ_INV_LEDGER_FREE": (1, 7 << 32 | 2)}
    assert int(clean["l_free"][1 * 3 + 2]) == 0   # two tasks of 0x9000... each on a total of 0x7000...: the sum saturates, nothing is left


def test_parts_select_and_absent_structures_are_skipped(clean):
    st = ac.corrupted("ledger_free")
    assert _three_orders(st, abi.HQ_CHECK_READY | abi.HQ_CHECK_GRAPH)["failed"] == {}
    no_ledger = dict(st, have=ac.HAVE_READY | ac.HAVE_GRAPH)
    rep = _three_orders(no_ledger, abi.HQ_CHECK_ALL)
    assert rep["checked"] == abi.HQ_CHECK_READY | abi.HQ_CHECK_GRAPH | abi.HQ_CHECK_CROSS and rep["failed"] == {}
    assert ac.expect(no_ledger, abi.HQ_CHECK_ALL) == (rep["checked"], {})
    nothing = dict(clean, have=0)
    rep = _three_orders(nothing, ac.STRICT_ALL)
    assert rep["checked"] == 0 and rep["n_failed"] == 0
    # a placement that waits for its consume: the Retracting table already shows the tick's redirects, the ledger not yet -- the redirect side is not compared
    pending = dict(ac.corrupted("x_retracting_redirect"), have=clean["have"] & ~ac.HAVE_SETTLED)
    assert _three_orders(pending, abi.HQ_CHECK_ALL)["failed"] == {}
    lib = _testhooks.load()
    c, keep = ac.to_c(clean)
    r = abi.CheckReportC()
    assert lib.hqtick_debug_audit_host(C.byref(c), 32, 0, C.byref(r)) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_audit_host(C.byref(c), 1, 3, C.byref(r)) == abi.HQTICK_E_INVALID
    assert lib.hqtick_debug_audit_host(None, 1, 0, C.byref(r)) == abi.HQTICK_E_INVALID


def test_report_and_table_layouts_match_the_headers():
    """sizeof / offsetof from a compiled C probe of include/hqtick.h and include/hqtick_debug.h against the ctypes mirrors; the constants; the version is still 12"""
    pairs = {"hqtick_check_report": abi.CheckReportC, "hqtick_debug_audit_tables": ac.AuditTablesC}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "hqtick_debug.h"', "int main(void){"]
    for cname, cls in pairs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    for n in abi.HQ_INV_NAMES + ("HQ_INV_N", "HQ_CHECK_READY", "HQ_CHECK_LEDGER", "HQ_CHECK_GRAPH", "HQ_CHECK_CROSS", "HQ_CHECK_STRICT", "HQ_CHECK_ALL", "HQTICK_ABI_VERSION"):
        lines.append(f'printf("{n} %u\\n", (unsigned){n});')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = dict(l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l)
    for cname, cls in pairs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    for n in abi.HQ_INV_NAMES + ("HQ_INV_N", "HQ_CHECK_READY", "HQ_CHECK_LEDGER", "HQ_CHECK_GRAPH", "HQ_CHECK_CROSS", "HQ_CHECK_STRICT", "HQ_CHECK_ALL"):
        assert int(got[n]) == getattr(abi, n), n
    assert int(got["HQTICK_ABI_VERSION"]) == 12 == abi.HQTICK_ABI_VERSION
    assert _testhooks.load().hqtick_abi_version() == 12


def test_item_functions_under_asan_on_exact_size_tables():
    """tools/audit_core_asan.cpp: the same item functions over the consistent state and every corruption, under AddressSanitizer + UBSan, every table in a heap block
    of exactly its size, in the three orders.  A stand-alone program: nothing is loaded into this process."""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    runs = [("clean", ac.consistent(), ac.STRICT_ALL)] + [(n, ac.corrupted(n), ac.CASES[n][1]) for n in sorted(ac.CASES)]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "audit_core_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "audit_core_asan.cpp")])
        for name, st, parts in runs:
            path = os.path.join(d, name + ".bin")
            open(path, "wb").write(ac.dump(st))
            p = subprocess.run([exe, path, str(parts)], capture_output=True, text=True, timeout=120, env=env)
            assert p.returncode == 0, name + ": " + p.stdout[-1000:] + p.stderr[-4000:]
            checked, want = ac.expect(st, parts)
            blocks = p.stdout.strip().split("order ")[1:]
            assert len(blocks) == 3, p.stdout
            for blk in blocks:
                head, *rows = blk.strip().split("\n")
                assert head.split()[1:] == ["checked", str(checked), "n_failed", str(len(want))], (name, head)
                got = {abi.HQ_INV_NAMES[int(r.split()[0])]: (int(r.split()[1]), int(r.split()[2])) for r in rows}
                assert got == want, name
