"""The mapping plan with no HIP in sight (csrc/map_core.h): the take sequences, the per-key tables, the redirects, the prefill walk, the selection plan and the
output offsets, the packed small tables — the part of the tick that decides what K4 and K5 are told and how large the plan's buffer is.  No GPU needed."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_core_under_sanitizers():
    """tools/map_core_asan.cpp: a few hundred small random ticks (both forms of the counts, prefill sets in front of and inside the queues, Retracting tasks, the
    dense and the view form of the table, 1 and 3 shards) through the five stages and both packers, the plan's invariants checked on each (key sums, takes per
    request, monotone output offsets, records per shard, when a key may be stored worker-major, the packed plan within what small_words said), and each refusal with
    its code and text — under AddressSanitizer + UBSan, every table in an exact-size heap block.  A stand-alone program: nothing is loaded into this process."""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "map_core_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                               os.path.join(ROOT, "tools", "map_core_asan.cpp")])
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "checks ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
