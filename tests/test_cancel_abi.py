"""hqtick_cancel_tasks and its accessors (include/hqtick.h): the four added functions are declared, exported, bound in Python and in the Rust
binding, the ABI version stays 12, and a NULL context is refused.  No GPU needed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

from hyperqueue_amd import abi, build, core, tick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hqtick_cancel_tasks", "hqtick_cancel_last_messages", "hqtick_cancel_last_routes", "hqtick_cancel_last_ready_removed"]
KINDS = {"HQ_CANCEL_NONE": 0, "HQ_CANCEL_ASSIGNED": 1, "HQ_CANCEL_PREFILLED": 2, "HQ_CANCEL_MN": 3, "HQ_CANCEL_RETRACTING": 4, "HQ_CANCEL_REPEAT": 5}


def test_prototypes_are_declared_and_the_version_stays_12():
    h = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\((const )?hqtick_ctx \*ctx", h), n
    assert "#define HQTICK_ABI_VERSION 12u" in h and abi.HQTICK_ABI_VERSION == 12
    for name, value in KINDS.items():
        assert re.search(r"#define " + name + r"\s+" + str(value) + r"\b", h), name
        assert getattr(abi, name) == value
    d = open(os.path.join(ROOT, "include", "hqtick_debug.h")).read()
    assert re.search(r"\bint hqtick_debug_cancel_group\(", d)


def test_library_exports_the_new_symbols_and_nothing_undeclared():
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\s(hqtick_\w+)$", out, flags=re.M))
    for n in NEW:
        assert n in syms, n
    h = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    for s in syms:
        if s.startswith("hqtick_cancel"):
            assert re.search(r"\b" + s + r"\(", h), s  # absent from no header
    assert "hqtick_debug_cancel_group" not in syms  # the hook lives in the test library only
    out = subprocess.run(["nm", "-D", "--defined-only", build.TEST_LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\shqtick_debug_cancel_group$", out, flags=re.M)


def test_rust_binding_is_regenerated():
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "tools", "gen_rust_sys.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    text = open(os.path.join(ROOT, "integration", "hqtick_sys.rs")).read()
    assert text == gen.generate()
    for n in NEW:
        assert re.search(r"pub fn " + n + r"\(", text), n
    for name in KINDS:
        assert name in text, name


def test_python_bindings_exist():
    assert callable(tick.Tick.cancel_tasks)
    assert callable(core.SchedEnv.cancel_tasks)


def test_null_context_is_refused():
    lib = tick.load()
    lib.hqtick_cancel_tasks.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.hqtick_cancel_last_messages.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u32p), C.POINTER(abi.u32p), C.POINTER(abi.u64p)]
    lib.hqtick_cancel_last_routes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.u32p), C.POINTER(abi.u8p)]
    lib.hqtick_cancel_last_ready_removed.argtypes = [C.c_void_p]; lib.hqtick_cancel_last_ready_removed.restype = C.c_uint64
    ids = (C.c_uint64 * 2)(1, 2)
    assert lib.hqtick_cancel_tasks(None, 0, None) == abi.HQTICK_E_INVALID
    assert lib.hqtick_cancel_tasks(None, 2, ids) == abi.HQTICK_E_INVALID
    n = C.c_uint32(7); w, o, t = abi.u32p(), abi.u32p(), abi.u64p()
    assert lib.hqtick_cancel_last_messages(None, C.byref(n), C.byref(w), C.byref(o), C.byref(t)) == abi.HQTICK_E_INVALID
    assert n.value == 0 and not w and not o and not t  # empty lists
    assert lib.hqtick_cancel_last_messages(None, None, None, None, None) == abi.HQTICK_E_INVALID
    n = C.c_uint32(7); k = abi.u8p()
    assert lib.hqtick_cancel_last_routes(None, C.byref(n), C.byref(w), C.byref(k)) == abi.HQTICK_E_INVALID
    assert n.value == 0 and not w and not k
    assert lib.hqtick_cancel_last_ready_removed(None) == 0
