"""The placement's solvers with no HIP in sight (csrc/solve_core.h): the staged image of a k_block_solve launch, the emulated block solver on it, the deal of the class
blocks over the ranks of a sharded scheduler, and the small derivations around a solve.  No GPU needed."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_core_under_sanitizers():
    """tools/solve_core_asan.cpp: 400 random small launches through the layout (offsets on 8 bytes, the class tables on 16, regions in order, sizes equal to the closed
    form, the image packed into an exact-size heap block and read back) and through the emulation (packed and in place alike); ShardedBlocks over EmulatedBlocks on 1, 2,
    3 and 5 ranks — threads over an in-process all-gather — against the unsharded answer byte for byte, with the pass below min_classes, one rank's failed solver, a
    failed all-gather (nobody blocks: the program ends) and the share arithmetic; fake_worker_set, loaded_flags and tick_status on hand-written counts — under
    AddressSanitizer + UBSan.  A stand-alone program: nothing is loaded into this process."""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "solve_core_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", exe,
                               os.path.join(ROOT, "tools", "solve_core_asan.cpp")])
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "checks ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
