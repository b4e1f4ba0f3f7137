"""The pure host pieces of phase A (csrc/scan_core.h): the parts of the scan that decide buffer sizes and trust device output — the runs of a dense histogram, the
decode of the ordered view's run table, the choice of radix passes, the wave geometry.  No GPU needed."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_core_under_sanitizers():
    """tools/scan_core_asan.cpp: runs against a brute-force count, accepted and refused run tables (each refusal and its code), the pass choice on the four kinds of
    digit histogram, the geometry at the sizes where a rule starts to bind — under AddressSanitizer + UBSan, every table in an exact-size heap block.  A stand-alone
    program: nothing is loaded into this process."""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "scan_core_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                               os.path.join(ROOT, "tools", "scan_core_asan.cpp")])
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "checks ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
