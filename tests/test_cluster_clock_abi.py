"""Clock mode's C ABI (include/hqtick.h: hqtick_cluster_set_clock, hqtick_cluster_deadlines, hqtick_cluster_last_row_groups): declared, exported, bound in
Python and in the Rust binding; functions only, the version stays 12.  No GPU needed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

from hyperqueue_amd import abi, build, tick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hqtick_cluster_set_clock", "hqtick_cluster_deadlines", "hqtick_cluster_last_row_groups"]


def _declared(header, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"_[a-z0-9_]+)\s*\(", src)))


def test_prototypes_are_declared_and_the_version_stays_12():
    h = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    assert "int hqtick_cluster_set_clock(hqtick_ctx *ctx, int64_t now_ns);" in h
    assert "int hqtick_cluster_deadlines(const hqtick_ctx *ctx, uint32_t *n_workers, const int64_t **deadline_ns);" in h
    assert "uint32_t hqtick_cluster_last_row_groups(const hqtick_ctx *ctx);" in h
    assert "#define HQTICK_ABI_VERSION 12u" in h and abi.HQTICK_ABI_VERSION == 12
    assert tick.load().hqtick_abi_version() == 12


def test_exported_symbol_tables_still_equal_the_headers():
    from hyperqueue_amd import _testhooks

    lib = build.build()
    dyn = lambda path: sorted(l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", path]).decode().splitlines() if l.strip())
    product = sorted(set(_declared("hqtick.h", "hqtick") + _declared("hqwire.h", "hqwire")))
    assert dyn(lib) == product
    for n in NEW:
        assert n in product, n
    _testhooks.load()
    hooks = sorted(set(product + _declared("hqtick_debug.h", "hqtick") + _declared("hqtick_debug.h", "hqwire")))
    assert dyn(build.TEST_LIB) == hooks
    for n in ("hqtick_debug_clock_rows", "hqtick_debug_clock_deadline", "hqtick_debug_clock_remaining", "hqtick_debug_clock_launches"):
        assert n in hooks and n not in product, n


def test_rust_binding_has_the_new_functions():
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "tools", "gen_rust_sys.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    text = open(os.path.join(ROOT, "integration", "hqtick_sys.rs")).read()
    assert text == gen.generate()
    assert re.search(r"pub fn hqtick_cluster_set_clock\(ctx: \*mut HqtickCtx, now_ns: i64\) -> c_int;", text)
    for n in NEW:
        assert re.search(r"pub fn " + n + r"\(", text), n


def test_python_bindings_exist():
    for m in ("cluster_set_clock", "cluster_deadlines", "cluster_last_row_groups"):
        assert callable(getattr(tick.Tick, m)), m


def test_null_context_is_refused():
    lib = tick.load()
    lib.hqtick_cluster_set_clock.argtypes = [C.c_void_p, C.c_int64]
    lib.hqtick_cluster_deadlines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hqtick_cluster_last_row_groups.argtypes = [C.c_void_p]; lib.hqtick_cluster_last_row_groups.restype = C.c_uint32
    assert lib.hqtick_cluster_set_clock(None, 5) == abi.HQTICK_E_INVALID
    assert lib.hqtick_cluster_deadlines(None, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_cluster_last_row_groups(None) == 0
