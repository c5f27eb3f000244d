"""crass_fastx_find_names (names in, first record index out, on the host) against a Python dictionary {name: first index} on
designed FASTA / FASTQ texts, and the status codes of the host function and of the device entry points' checks that come before
any device call.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import crass_amd as ca
from tests import fastx_sets, header_sets, name_sets

TEXTS = name_sets.texts()
NF = name_sets.NOT_FOUND


def test_the_texts_are_what_they_say():
    lens = set()
    for name in ("lengths_fa", "lengths_fq"):
        data, rp = TEXTS[name]
        d = name_sets.first_by_name(data, rp)
        lens |= {len(k) for k in d}
        assert len(d) < len(rp) - 1                      # names repeat
    assert lens >= set(name_sets.LENGTHS)
    data, rp = TEXTS["tail_260"]
    assert int(rp[-2]) + 1 + 260 == len(data) and data[-1:] not in (b"\n",)
    d = name_sets.first_by_name(*TEXTS["cuts"])
    assert d[b"x"] == 0 and d[b"xy"] == 4 and d[b"x\x0ey"] == 5 and d[b"cut"] == 7 and d[b"crlf"] == 10 and d[b""] == 12
    assert name_sets.first_by_name(*TEXTS["prefixes"])[b"read10"] == 1
    assert name_sets.first_by_name(*TEXTS["tail_empty_name"])[b""] == 1
    assert any(max(k) >= 0x80 for k in name_sets.first_by_name(*TEXTS["high_bytes"]) if k)


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_find_equals_the_dictionary(name):
    data, rp = TEXTS[name]
    q = name_sets.queries(data, rp)
    want = name_sets.expected(data, rp, q)
    got = ca.find_names(data, rp, q)
    assert got.dtype == np.uint64 and np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5])
    d = name_sets.first_by_name(data, rp)
    assert all(int(got[k]) == d[q[k]] for k in range(len(d)))      # every present name is found
    assert np.count_nonzero(got == NF) > len(d)                       # ... and the variants are not


def test_scanned_inputs_and_header_ids_agree():
    """on accepted inputs: find(name of record r) is header_id[r]"""
    inputs = dict(fastx_sets.regular(), **header_sets.designed())
    for name, data in sorted(inputs.items()):
        lay = ca.fastx_scan_host(data)
        assert lay.accepted, name
        hid = ca.fastx_header_ids(data, lay.rec_pos)
        names = [name_sets.name_at(data, int(p)) for p in lay.rec_pos[:-1]]
        assert np.array_equal(ca.find_names(data, lay.rec_pos, names), hid), name
        q = name_sets.queries(data, lay.rec_pos)[:400]
        assert np.array_equal(ca.find_names(data, lay.rec_pos, q), name_sets.expected(data, lay.rec_pos, q)), name


def test_queries_as_arrays_at_any_offset():
    data, rp = TEXTS["prefixes"]
    q = name_sets.queries(data, rp)
    want = name_sets.expected(data, rp, q)
    for lead in range(4):
        chars, off = name_sets.concat(q)
        chars = np.concatenate([np.full(lead, 0x41, np.uint8), chars])
        assert np.array_equal(ca.find_names(data, rp, (chars, off + np.uint64(lead))), want), lead


def test_no_queries_and_no_records():
    data, rp = TEXTS["repeats"]
    assert len(ca.find_names(data, rp, [])) == 0
    none = np.zeros(1, np.uint64)
    got = ca.find_names(b"", none, [b"", b"a", b"a b"])
    assert got.tolist() == [NF, NF, NF]
    got = ca.find_names(data, rp[:1], [b"a"])             # bytes, but no records
    assert got.tolist() == [NF]


def test_status_codes():
    lib = ca.load()
    fn = lib.crass_fastx_find_names
    data, rp = TEXTS["repeats"]
    a = np.frombuffer(data, np.uint8)
    n = len(rp) - 1
    chars, off = name_sets.concat([b"a", b"dd", b"zz"])
    out = np.full(3, 7, np.uint64)
    args = lambda **kw: [kw.get("bytes", a.ctypes.data), kw.get("n_bytes", len(a)), kw.get("rec_pos", rp.ctypes.data), kw.get("n_reads", n),
                         kw.get("names", chars.ctypes.data), kw.get("name_off", off.ctypes.data), kw.get("n_names", 3), kw.get("out", out.ctypes.data)]
    assert fn(*args()) == 0 and out.tolist() == [0, 6, NF]
    out[:] = 7
    assert fn(*args(bytes=None)) == 1 and fn(*args(rec_pos=None)) == 1 and fn(*args(names=None)) == 1
    assert fn(*args(name_off=None)) == 1 and fn(*args(out=None)) == 1
    down = np.asarray([0, 3, 1, 5], np.uint64)
    assert fn(*args(name_off=down.ctypes.data)) == 1
    bad = rp.copy()
    bad[n // 2] = len(a)
    assert fn(*args(rec_pos=bad.ctypes.data)) == 1
    assert np.all(out == 7)
    assert fn(*args(n_names=0, names=None, name_off=None, out=None)) == 0
    assert fn(None, 0, None, 0, chars.ctypes.data, off.ctypes.data, 3, out.ctypes.data) == 0 and out.tolist() == [NF] * 3
    empties = np.zeros(3, np.uint64)
    assert fn(*args(names=None, name_off=empties.ctypes.data, n_names=2)) == 0      # empty queries need no bytes
    assert C.c_uint64(NF).value == ca._abi.NAME_NOT_FOUND


def test_the_device_entry_points_check_their_arguments_first():
    lib = ca.load()
    rp = np.asarray([0, 5, 10], np.uint64)
    chars, off = name_sets.concat([b"a"])
    out = np.full(1, 7, np.uint64)
    assert lib.crass_hip_fastx_names_build_device(None, 16, 10, rp.ctypes.data, 2) == 1
    assert lib.crass_hip_fastx_names_find(None, chars.ctypes.data, off.ctypes.data, 1, out.ctypes.data) == 1
    assert lib.crass_hip_fastx_names_drop(None) == 1
    assert lib.crass_hip_last_names_ms(None, 0) == 0.0
    assert np.all(out == 7)
    import inspect
    from crass_amd import distributed
    assert inspect.isclass(distributed.FoundNameExchange)
    assert all(hasattr(ca.SearchEngine, m) for m in ("names_build", "names_find", "names_drop"))
