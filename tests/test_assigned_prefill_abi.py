"""Prefilled tasks in the assignment ledger (include/hqtick.h): the five added functions are declared, exported, bound in Python and in
the Rust binding, and the ABI version stays 12.  No GPU needed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

from hyperqueue_amd import abi, build, tick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hqtick_assigned_track_prefilled", "hqtick_assigned_start_prefilled", "hqtick_assigned_unprefill", "hqtick_assigned_prefilled_count",
       "hqtick_cluster_last_requeued_prefilled"]


def test_prototypes_are_declared_and_the_version_stays_12():
    h = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\((const )?hqtick_ctx \*ctx", h), n
    assert "#define HQTICK_ABI_VERSION 12u" in h and abi.HQTICK_ABI_VERSION == 12
    assert "PREFILL records and prefill sets stay the host's" not in h


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


def test_python_bindings_exist():
    for m in ["assigned_track_prefilled", "assigned_start_prefilled", "assigned_unprefill", "assigned_prefilled_count", "cluster_last_requeued_prefilled"]:
        assert callable(getattr(tick.Tick, m)), m


def test_null_context_is_refused():
    lib = tick.load()
    lib.hqtick_assigned_track_prefilled.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hqtick_assigned_start_prefilled.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.hqtick_assigned_unprefill.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.hqtick_assigned_prefilled_count.argtypes = [C.c_void_p]; lib.hqtick_assigned_prefilled_count.restype = C.c_uint64
    lib.hqtick_cluster_last_requeued_prefilled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.hqtick_assigned_track_prefilled(None, 0, None, None, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_assigned_start_prefilled(None, 0, None, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_assigned_unprefill(None, 0, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_assigned_prefilled_count(None) == 0
    assert lib.hqtick_cluster_last_requeued_prefilled(None, None, None) == abi.HQTICK_E_INVALID
