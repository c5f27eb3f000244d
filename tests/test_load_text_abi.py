"""CPU-side checks of the device packer's boundary (crass_hip_load_text / crass_hip_attach_device_text /
crass_hip_get_packed): the three entry points are exported and declared, the byte -> code function the kernel and the
host share is exact for all 256 byte values in every byte position, and the layout (stride / uniform length) the new
calls give a read set is the one crass_pack_reads gives it.  No GPU is needed."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from tests import text_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def test_entry_points_exported_and_declared(ca):
    lib = C.CDLL(ca.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "crass_hip.h")).read()
    for name in ("crass_hip_load_text", "crass_hip_attach_device_text", "crass_hip_get_packed"):
        assert hasattr(lib, name), "missing export: " + name
        assert name in ca.SYMBOLS, "no prototype in _abi.py: " + name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), "not declared in crass_hip.h: " + name
    assert ca.SYMBOLS["crass_hip_load_text"][1] == ca.SYMBOLS["crass_hip_attach_device_text"][1]
    assert len(ca.SYMBOLS["crass_hip_load_text"][1]) == 7
    assert ca.load().crass_hip_abi_version() == 3
    from crass_amd import _abi
    assert _abi.ABI_VERSION == 3 and "#define CRASS_HIP_ABI_VERSION 3" in hdr
    assert hasattr(lib, "crass_hip_last_pack_ms") and "crass_hip_last_pack_ms" in ca.SYMBOLS
    for method in ("load_text", "attach_device_text", "packed", "last_pack_ms"):
        assert callable(getattr(ca.SearchEngine, method))


def test_code_function_is_exact_for_every_byte_in_every_position(ca):
    """ACGT -> 0..3 and no flag; every other value -> code 0 and the flag, incl. acgt, N, U, 0x00, 0xFF — the table semantics of
    crass_pack_reads (ingest.cpp).  Every value in each of the four byte positions, seeded random bytes in the other three."""
    want = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    rng = random.Random(20261017)
    checked = 0
    for pos in range(4):
        for value in range(256):
            for _ in range(8):
                b = [rng.randrange(256) for _ in range(4)]
                if rng.random() < 0.5:                   # (half of the neighbours are letters: both kinds beside every value)
                    b = [rng.choice(b"ACGT") if rng.random() < 0.8 else x for x in b]
                b[pos] = value
                word = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24)
                code, bad = ca.pack_code4(word)
                assert code < 256 and bad < 16
                for i in range(4):
                    exp_code, exp_bad = (want[b[i]], 0) if b[i] in want else (0, 1)
                    assert (code >> (2 * i)) & 3 == exp_code, (pos, value, b, i)
                    assert (bad >> i) & 1 == exp_bad, (pos, value, b, i)
                checked += 1
    assert checked == 4 * 256 * 8
    for ch in b"acgtNnU\x00\xff":
        assert ca.pack_code4(ch | (ord("A") << 8) | (ord("A") << 16) | (ord("A") << 24)) == (0, 1)
    assert ca.pack_code4(int.from_bytes(b"ACGT", "little")) == (0b11100100, 0)


def _layout_rule(lengths, pad):
    """the rule of include/crass_hip.h (crass_pack_reads), restated: (stride_words, uniform_len)"""
    n = len(lengths)
    mx, mn = (max(lengths), min(lengths)) if n else (0, 0)
    uniform = n > 0 and mx == mn and mx > 0
    if pad == 2:
        tight = sum((l + 15) // 16 for l in lengths)
        pad = 1 if (64 <= mx <= 256 and n * ((mx + 15) // 16) <= 2 * tight) else 0
    stride = max(1, (mx + 15) // 16) if (pad or uniform) else 0
    return stride, (mx if uniform else 0)


@pytest.mark.parametrize("name", text_sets.LAYOUT_SETS)
@pytest.mark.parametrize("pad", [0, 1, 2])
def test_layout_decision_is_crass_pack_reads_decision(ca, name, pad):
    """crass_pack_layout wraps crass::pack_layout, the function crass_hip_load_text / crass_hip_attach_device_text decide with.
    crass_pack_reads calls the same function since it was factored out, so comparing the two alone would compare a function
    with itself: the expected values come from the rule restated in Python above, and crass_pack_reads' own result (whose
    layouts the older tests of tests/test_abi.py pin) must agree with both."""
    seqs = text_sets.make(ca, name)
    buf, off = text_sets.concat(seqs)
    want = _layout_rule([len(s) for s in seqs], pad)
    pk = ca.PackedReads((buf, off), pad_uniform=pad)
    assert (int(pk.reads.stride_words), int(pk.reads.uniform_len)) == want, name
    assert ca.pack_layout(off, pad) == want, name
    assert ca.pack_layout(off + np.uint64(13), pad) == want           # (the decision depends on lengths only)


def test_layout_errors(ca):
    lib = ca.load()
    off = np.array([0, 10, 5], dtype=np.uint64)
    assert lib.crass_pack_layout(off.ctypes.data, 2, 0, None, None) == 1          # CRASS_ERR_INVALID_ARG: offsets decrease
    off = np.array([0, 60001], dtype=np.uint64)
    assert lib.crass_pack_layout(off.ctypes.data, 1, 2, None, None) == 2          # CRASS_ERR_UNSUPPORTED
    assert lib.crass_pack_layout(None, 3, 0, None, None) == 1
    assert lib.crass_pack_layout(None, 0, 0, None, None) == 0
    # the host packer keeps its own answer for such offsets
    from crass_amd import _abi
    p = _abi.Packed()
    buf = np.zeros(16, np.uint8)
    bad = np.array([0, 10, 5], dtype=np.uint64)
    assert lib.crass_pack_reads(buf.ctypes.data, bad.ctypes.data, 2, 0, C.byref(p)) == 2
