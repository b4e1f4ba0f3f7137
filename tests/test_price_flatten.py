"""The coupled solve's flatteners with no HIP in sight (csrc/price_flatten.cpp): a component (hqprice::Request) or the model as its builder wrote it
(hqprice::ModelView) -> blocks + wide rows (csrc/price_prob.h: Prob), one set of steps for both forms.  No GPU needed."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_price_flatten_under_sanitizers():
    """tools/price_flatten_asan.cpp: hand-written models of 8 to 11 blocks in both forms — the smallest accepted model against a written-out table of every array of
    Prob and HostTables; one model per refusal text, in every form the text exists in; rows that are passed over (implied, vacuous, holding at zero, empty) and a
    duplicate term that is summed; a block with 4 rows and one left with the never-binding row; a conditional bound with two flags and a `>=` wide row with a flag;
    the grouping of wide rows (one left-hand side with two signs, two equal shared lists, an own list with a shared list's content); equal-block runs (one that
    holds, one that fails in its last block, one at the model's end, one whose first block is not fresh), each against the same model without block_runs; the
    after_blocks hook (called once, the eight block arrays final); and for every accepted model the Request made of the same rows, unscaled and with every second
    row scaled by 2, which must leave the same digest — under AddressSanitizer + UBSan, every input array in an exact-size heap block.  A stand-alone program:
    nothing is loaded into this process."""
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "price_flatten_asan")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                               os.path.join(ROOT, "tools", "price_flatten_asan.cpp"), os.path.join(ROOT, "hyperqueue_amd", "csrc", "price_flatten.cpp")])
        p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "checks ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
