"""hqtick_assigned_last_host_bytes (include/hqtick.h): how a host sees that a tick's records stayed on the device when its placement entered the assignment
ledger.  Declared, exported, bound in Python and in the generated Rust binding; the ABI version is unchanged.  No GPU needed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

from hyperqueue_amd import abi, build, tick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GETTER = "hqtick_assigned_last_host_bytes"


def test_getter_is_declared_and_the_abi_version_stays():
    h = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    assert re.search(r"\buint64_t " + GETTER + r"\(const hqtick_ctx \*ctx\);", h)
    assert "#define HQTICK_ABI_VERSION 12u" in h and abi.HQTICK_ABI_VERSION == 12


def test_getter_is_exported():
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert GETTER in set(re.findall(r"\s(hqtick_\w+)$", out, flags=re.M))


def test_getter_is_in_the_regenerated_rust_binding():
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "tools", "gen_rust_sys.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    text = open(os.path.join(ROOT, "integration", "hqtick_sys.rs")).read()
    assert text == gen.generate()
    assert re.search(r"pub fn " + GETTER + r"\(ctx: \*const HqtickCtx\) -> u64;", text)


def test_python_bindings_exist():
    assert callable(tick.Tick.assigned_last_host_bytes) and callable(tick.Tick.set_record_sink)


def test_null_context_gives_zero():
    lib = tick.load()
    f = getattr(lib, GETTER)
    f.argtypes = [C.c_void_p]; f.restype = C.c_uint64
    assert f(None) == 0


def test_the_ledger_no_longer_refuses_an_emission_form_in_the_header():
    """the header is the contract a host reads: compact records and a record sink are allowed with the ledger, sharded and replica contexts are not"""
    h = open(os.path.join(ROOT, "include", "hqtick.h")).read()
    doc = h[h.index("hqtick_assigned_last_host_bytes  bytes of record data"):h.index("int hqtick_assigned_enable(")]
    assert "HQTICK_E_UNSUPPORTED on a sharded or replica context" in doc and "record sink)" not in doc
