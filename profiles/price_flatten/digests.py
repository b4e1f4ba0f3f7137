"""What the coupled tick's host stages make of a fixed list of snapshots, one line per case and path, with the price sweeps emulated on the CPU
(hqtick_debug_set_price_emulation(1, 64)).  Not a test: run on two builds (each in a tree of its own, this file copied into it) and compared with cmp — see README.md.

  fast path     the four values of hqtick_debug_last_coupled_digest (model, flattened problem and tables, runs recorded, blocks the runs covered), sweeps, rounds,
                a hash of the first cut's bytes, status, is_optimal, a hash of the counts
  classic path  (hqtick_debug_set_fast_path(0)) the same without the digest and the first cut, which the component path does not keep

Cases: every case of tests/test_block_runs.py with the runs on and off, the five FAST_CASES of tests/test_price.py, the eight parameter sets of
test_heterogeneous_coupled_ticks_by_price_sweeps.

    python profiles/price_flatten/digests.py > digests.txt
"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_block_runs as tbr  # noqa: E402
import test_price as tp  # noqa: E402
from host_stages import HostStages  # noqa: E402
from hyperqueue_amd import abi  # noqa: E402

HETERO = [(16, 1, 120, 1), (24, 2, 200, 2), (32, 3, 150, 3), (48, 4, 400, 1), (64, 5, 300, 2), (64, 6, 900, 3), (96, 7, 500, 1), (128, 8, 700, 2)]


def h(obj) -> str:
    return hashlib.sha1(obj if isinstance(obj, bytes) else repr(obj).encode()).hexdigest()[:16]


def line(name: str, snap, fast: bool, runs: int, corrupt: bool = False) -> str:
    hs = HostStages(abi.make_config(time_limit_s=20.0))
    lib = tbr._lib(hs)
    lib.hqtick_debug_set_fast_path.argtypes = [C.c_int]
    lib.hqtick_debug_capture_first_cut.argtypes = [C.c_int]
    lib.hqtick_debug_first_cut.argtypes = [C.c_char_p, C.c_uint32]
    lib.hqtick_debug_first_cut.restype = C.c_uint32
    lib.hqtick_debug_set_price_emulation(1, 64)
    lib.hqtick_debug_set_fast_path(1 if fast else 0)
    lib.hqtick_debug_set_block_runs(runs)
    lib.hqtick_debug_capture_first_cut(1)
    lib.hqtick_debug_corrupt_block_runs(1 if corrupt else 0)  # (tests/test_block_runs.py: test_a_false_run_is_refused)
    try:
        got = hs.stages(snap)
        buf = C.create_string_buffer(1 << 20)
        cut = buf.raw[:lib.hqtick_debug_first_cut(buf, len(buf))]
    finally:
        lib.hqtick_debug_set_price_emulation(0, 0)
        lib.hqtick_debug_set_fast_path(-1)
        lib.hqtick_debug_set_block_runs(-1)
        lib.hqtick_debug_capture_first_cut(0)
        lib.hqtick_debug_corrupt_block_runs(0)
    d = (C.c_uint64 * 4)()
    lib.hqtick_debug_last_coupled_digest(d)
    sw, rd = C.c_uint32(), C.c_uint32()
    lib.hqtick_debug_last_price(C.byref(sw), C.byref(rd))
    tail = f"sweeps {sw.value} rounds {rd.value} status {got.status} optimal {int(bool(got.is_optimal))} counts {h([list(map(int, c)) for c in got.counts])}"
    if not fast:
        return f"{name} classic {tail}"
    return f"{name} fast runs={runs} digest {d[0]:016x} {d[1]:016x} {d[2]} {d[3]} first_cut {h(cut)}/{len(cut)} {tail}"


def main() -> None:
    cases = [("block_runs/" + c[0], c[1]) for c in tbr.CASES] + [("block_runs/few_tasks", lambda: tbr.few_tasks(64, 600))]
    for name, make in cases:
        snap = make()
        for runs in (1, 0):
            print(line(name, snap, True, runs), flush=True)
        print(line(name, snap, False, 1), flush=True)
    print(line("block_runs/two_halves_false_run", tbr.halves(32), True, 1, corrupt=True), flush=True)
    others = [("fast/" + k, tp.FAST_CASES[k]) for k in sorted(tp.FAST_CASES)] + [("hetero/%d-%d-%d-%d" % p, (lambda p=p: tp.steady_coupled(*p))) for p in HETERO]
    for name, make in others:
        snap = make()
        print(line(name, snap, True, 1), flush=True)
        print(line(name, snap, False, 1), flush=True)


if __name__ == "__main__":
    main()
