"""The fetch of read text out of the resident set (crass_hip_fetch_text and its four companions), without a GPU: the symbols
are exported, declared and bound, the ABI version has not moved, and the argument checks that come before any device call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH_SYMBOLS = ("crass_hip_fetch_text", "crass_hip_fetch_text_device", "crass_hip_fetch_record_text", "crass_hip_group_fetch_text",
                 "crass_hip_last_fetch_ms")
INVALID_ARG = 1


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def test_symbols_are_exported_declared_and_bound(ca):
    hdr = open(os.path.join(ROOT, "include", "crass_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(crass_[a-z_0-9]+)\s*\(", hdr))
    raw = C.CDLL(ca.LIB_PATH)
    for name in FETCH_SYMBOLS:
        assert name in declared, name
        assert hasattr(raw, name), "missing export: " + name
        assert name in ca.SYMBOLS, name
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*crass_text\s*;", hdr)


def test_abi_version_is_still_3(ca):
    hdr = open(os.path.join(ROOT, "include", "crass_hip.h")).read()
    assert re.search(r"#define\s+CRASS_HIP_ABI_VERSION\s+3\b", hdr)
    assert ca.load().crass_hip_abi_version() == 3


def test_null_context_and_null_result_are_refused_before_any_device_call(ca):
    """a NULL context, and a NULL result pointer, from every entry point.  The result pointer is checked before the context is
    looked at, so the second half can pass a handle that is no context: 4 KB of zeros that nothing may read as one"""
    from crass_amd import _abi
    lib = ca.load()
    idx = (C.c_uint64 * 2)(0, 1)
    off = (C.c_uint64 * 3)()
    t = _abi.Text()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    assert lib.crass_hip_fetch_text(None, idx, None, 2, C.byref(t)) == INVALID_ARG
    assert lib.crass_hip_fetch_text(h, idx, None, 2, None) == INVALID_ARG
    assert lib.crass_hip_fetch_text_device(None, idx, None, 2, None, 0, off) == INVALID_ARG
    assert lib.crass_hip_fetch_text_device(h, idx, None, 2, None, 0, None) == INVALID_ARG
    for p in (0, 1, 2, 3):
        assert lib.crass_hip_fetch_record_text(None, p, C.byref(t)) == INVALID_ARG
    assert lib.crass_hip_fetch_record_text(h, 1, None) == INVALID_ARG
    assert lib.crass_hip_group_fetch_text(None, idx, None, 2, C.byref(t)) == INVALID_ARG
    assert lib.crass_hip_group_fetch_text(h, idx, None, 2, None) == INVALID_ARG
    assert lib.crass_hip_last_fetch_ms(None) == 0.0
    assert fake.raw == b"\0" * 4096


def test_python_methods_exist(ca):
    for name in ("fetch_text", "fetch_record_text", "last_fetch_ms"):
        assert callable(getattr(ca.SearchEngine, name)), name
    assert callable(ca.SearchGroup.fetch_text)
    assert hasattr(ca, "Text") and hasattr(ca.Text, "__getitem__")
