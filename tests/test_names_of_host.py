"""The names of listed records, back to back (crass_fastx_names_of; host, no GPU) against name_sets.name_at on every designed
text: records in any order with repeats, both index bases, n of 0 and 1, the capacity one byte short, exact and one byte long
with the bytes behind it left alone, and an index out of range."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import name_sets

TEXTS = name_sets.texts()
FILL = 0xA5


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def picks(name, n_reads):
    """record numbers in any order, with repeats, every record at least once"""
    rng = random.Random("names_of:" + name)
    idx = list(range(n_reads)) + [rng.randrange(n_reads) for _ in range(n_reads + 5)]
    rng.shuffle(idx)
    return idx


def want_of(data, rp, idx):
    names = [name_sets.name_at(data, int(rp[r])) for r in idx]
    return name_sets.concat(names)


def raw(ca, data, rp, idx, base, cap, guard=8):
    """the C call itself into a buffer of cap bytes with a guard of FILL bytes behind it: (status, buffer, offsets)"""
    a = np.frombuffer(data, np.uint8)
    ix = np.asarray(idx, np.uint64) + np.uint64(base)
    out = np.full(cap + guard, FILL, np.uint8)
    off = np.full(len(ix) + 1, 2 ** 64 - 1, np.uint64)
    st = ca.load().crass_fastx_names_of(a.ctypes.data if len(a) else None, len(a), rp.ctypes.data, len(rp) - 1, ix.ctypes.data if len(ix) else None,
                                        len(ix), base, out.ctypes.data, cap, off.ctypes.data)
    return st, out, off


@pytest.mark.parametrize("base", [0, 7])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_names_equal_name_at(ca, name, base):
    data, rp = TEXTS[name]
    idx = picks(name, len(rp) - 1)
    chars, off = want_of(data, rp, idx)
    got_c, got_o = ca.names_of(data, rp, np.asarray(idx, np.uint64) + np.uint64(base), idx_base=base)
    assert np.array_equal(got_o, off) and np.array_equal(got_c, chars), name
    total = int(off[-1])
    for cap in (total - 1, total, total + 1):
        if cap < 0:
            continue
        st, out, o = raw(ca, data, rp, idx, base, cap)
        assert st == (8 if cap < total else 0), (name, cap)
        assert np.array_equal(o, off)                                          # the offsets are complete either way
        m = min(cap, total)
        assert np.array_equal(out[:m], chars[:m]) and np.all(out[m:] == FILL), (name, cap)


@pytest.mark.parametrize("name", ["lengths_fa", "cuts", "tail_empty_name", "tail_only"])
def test_none_and_one(ca, name):
    data, rp = TEXTS[name]
    st, out, off = raw(ca, data, rp, [], 0, 0)
    assert st == 0 and off.tolist() == [0] and np.all(out == FILL)
    for r in range(len(rp) - 1):
        nm = name_sets.name_at(data, int(rp[r]))
        for base in (0, 7):
            st, out, off = raw(ca, data, rp, [r], base, len(nm))
            assert st == 0 and off.tolist() == [0, len(nm)] and bytes(out[:len(nm)]) == nm and np.all(out[len(nm):] == FILL)


def test_an_index_out_of_range(ca):
    data, rp = TEXTS["prefixes"]
    n = len(rp) - 1
    for idx, base in (([0, n], 0), ([n + 6, n + 7], 7), ([2, 6], 7), ([2 ** 64 - 8], 7), ([3, 2 ** 63], 0)):
        a = np.frombuffer(data, np.uint8)
        ix = np.asarray(idx, np.uint64)
        out = np.full(4096, FILL, np.uint8)
        off = np.zeros(len(ix) + 1, np.uint64)
        st = ca.load().crass_fastx_names_of(a.ctypes.data, len(a), rp.ctypes.data, n, ix.ctypes.data, len(ix), base, out.ctypes.data, len(out), off.ctypes.data)
        assert st == 1 and np.all(out == FILL), (idx, base)
    with pytest.raises(ca.CrassError) as err:
        ca.names_of(data, rp, [n])
    assert err.value.status == 1
    # NULL arrays with counts > 0, a NULL offsets array
    lib = ca.load()
    off = np.zeros(2, np.uint64)
    ix = np.zeros(1, np.uint64)
    a = np.frombuffer(data, np.uint8)
    assert lib.crass_fastx_names_of(a.ctypes.data, len(a), rp.ctypes.data, n, None, 1, 0, None, 0, off.ctypes.data) == 1
    assert lib.crass_fastx_names_of(a.ctypes.data, len(a), rp.ctypes.data, n, ix.ctypes.data, 1, 0, None, 0, None) == 1
    assert lib.crass_fastx_names_of(None, len(a), rp.ctypes.data, n, ix.ctypes.data, 1, 0, None, 0, off.ctypes.data) == 1
    assert lib.crass_fastx_names_of(a.ctypes.data, len(a), rp.ctypes.data, n, ix.ctypes.data, 1, 0, None, 5, off.ctypes.data) == 1
