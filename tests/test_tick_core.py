"""The tick's host stages with no HIP in sight (csrc/tick_core.h): the snapshot's checks, the scan table of a histogram and the queue levels, the batches' export,
the plan's input and stage sequence, the retry around a deferred row check, a query's tail — the one implementation the tick, the queries and the CPU test hooks
run.  No GPU needed."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tick_core_under_sanitizers():
    """tools/tick_core_asan.cpp: validate on one hand-written snapshot per refusal text, the smallest valid snapshot and the empty edges (W = 0, Q = 0, n_ready = 0);
    table_from_hist and queue_levels on a 3-level x 2-request histogram with a zero cell, with a prefill set that merges into the top level and one that goes in
    front; export_batches on batches with 0, 1 and 2 cuts and 0 to 2 blockers (offset arrays monotone, ending at their arrays' sizes); with_row_check on a stub pass
    (nothing pending, pending and passing, pending and failing with the counts reset before the classic pass, an error beside a failing check, a check the pass
    settled itself, a failing discard) with the row checks counted; plan_stages on a stub `after` (0, 1, 2, 3 in order, a non-zero answer ends the sequence with its
    code, a stage's refusal with the stage's text); query_tail with two fake workers, one request and a stub solve that loads worker 1 — under AddressSanitizer +
    UBSan, every array in an exact-size heap block.  A stand-alone program: nothing is loaded into this process."""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tick_core_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                               os.path.join(ROOT, "tools", "tick_core_asan.cpp")])
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "checks ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
