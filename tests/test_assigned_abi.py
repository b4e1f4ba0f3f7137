"""The assignment ledger's C ABI (ABI 12; include/hqtick.h): declared, exported, bound in Python and in the Rust binding.  No GPU needed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

from hyperqueue_amd import abi, build, tick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hqtick_assigned_enable", "hqtick_assigned_disable", "hqtick_assigned_add", "hqtick_assigned_release", "hqtick_assigned_last_unknown",
       "hqtick_assigned_count", "hqtick_assigned_lookup", "hqtick_assigned_free_rows", "hqtick_cluster_last_requeued"]


def _header():
    return open(os.path.join(ROOT, "include", "hqtick.h")).read()


def test_prototypes_are_declared():
    h = _header()
    for n in NEW:
        assert re.search(r"\b" + n + r"\(hqtick_ctx \*ctx|\b" + n + r"\(const hqtick_ctx \*ctx", h), n
    assert "#define HQTICK_ABI_VERSION 12u" in h and abi.HQTICK_ABI_VERSION == 12


def test_library_exports_the_new_symbols():
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\s(hqtick_\w+)$", out, flags=re.M))
    for n in NEW:
        assert n in syms, n


def test_rust_binding_has_the_new_functions():
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "tools", "gen_rust_sys.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    text = open(os.path.join(ROOT, "integration", "hqtick_sys.rs")).read()
    assert text == gen.generate()
    for n in NEW:
        assert re.search(r"pub fn " + n + r"\(", text), n


def test_configs_of_abi_10_and_11_are_still_accepted():
    """hqtick_create checks the version before it looks for a device: 10, 11 and 12 get past the check (NO_DEVICE here, or a context on a GPU);
    anything else is INVALID"""
    lib = tick.load()
    lib.hqtick_create.argtypes = [C.POINTER(abi.Config), C.POINTER(C.c_void_p)]
    lib.hqtick_destroy.argtypes = [C.c_void_p]
    for v, ok in ((10, True), (11, True), (12, True), (9, False), (13, False)):
        cfg = abi.make_config(); cfg.abi_version = v
        ctx = C.c_void_p()
        rc = lib.hqtick_create(C.byref(cfg), C.byref(ctx))
        if ctx.value:
            lib.hqtick_destroy(ctx)
        assert (rc != abi.HQTICK_E_INVALID) == ok, (v, rc)


def test_python_bindings_exist():
    for m in ["assigned_enable", "assigned_disable", "assigned_add", "assigned_release", "assigned_last_unknown", "assigned_count", "assigned_lookup",
              "assigned_free_rows", "cluster_last_requeued"]:
        assert callable(getattr(tick.Tick, m)), m


def test_null_context_is_refused():
    lib = tick.load()
    lib.hqtick_assigned_release.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.hqtick_assigned_count.argtypes = [C.c_void_p]; lib.hqtick_assigned_count.restype = C.c_uint64
    assert lib.hqtick_assigned_release(None, 0, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_assigned_count(None) == 0
