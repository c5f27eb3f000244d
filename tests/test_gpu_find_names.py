"""Names in, first record index out, from a name table kept on the device (crass_hip_fastx_names_build_device / _find / _drop,
k_hid_find and k_hid_find_long of fastx_hid.hip) against the host's crass_fastx_find_names on the same bytes, element for
element: designed names, probe chains under a cut hash (CRASS_HID_TEST_HASH_BITS), every alignment of the bytes and of the
queries, lane and wave kernel on both sides, the files route, errors, and the header ids of the same context left as they were."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from tests import bgzf_sets, fastx_sets, name_sets

pytestmark = pytest.mark.gpu

TEXTS = name_sets.texts()
NF = name_sets.NOT_FOUND


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def eng(ca):
    with ca.SearchEngine() as e:
        yield e


def device_copy(data, lead=0):
    """the bytes in a device tensor that starts `lead` bytes behind an aligned allocation, name bytes all around them: a read
    beyond the input makes its last name longer"""
    import torch
    big = torch.full((len(data) + lead + 64,), 0x51, dtype=torch.uint8, device="cuda")
    t = big[lead:lead + len(data)]
    if len(data):
        t.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    assert t.data_ptr() % 4 == lead % 4
    return big, t


def engine_with_hash_bits(ca, bits):
    old = os.environ.pop("CRASS_HID_TEST_HASH_BITS", None)
    if bits is not None:
        os.environ["CRASS_HID_TEST_HASH_BITS"] = str(bits)
    try:
        return ca.SearchEngine()                          # (the switch is read when the context is created)
    finally:
        os.environ.pop("CRASS_HID_TEST_HASH_BITS", None)
        if old is not None:
            os.environ["CRASS_HID_TEST_HASH_BITS"] = old


def shifted(q, lead):
    """the queries as arrays, `lead` bytes of something else in front of them"""
    chars, off = name_sets.concat(q)
    return np.concatenate([np.full(lead, 0x51, np.uint8), chars]), off + np.uint64(lead)


_want = {}


def want_of(ca, key, data, rp, q):
    """the host function's answer: once per input"""
    if key not in _want:
        w = ca.find_names(data, rp, q)
        assert np.array_equal(w, name_sets.expected(data, rp, q)), key
        _want[key] = w
    return _want[key]


def check(ca, e, key, data, rp, lead=0, qlead=0, q=None):
    q = name_sets.queries(data, rp) if q is None else q
    want = want_of(ca, key, data, rp, q)
    big, t = device_copy(data, lead)
    e.names_build(t, rp)
    got = e.names_find(shifted(q, qlead) if qlead else q)
    assert got.dtype == np.uint64 and np.array_equal(got, want), (key, lead, qlead, np.flatnonzero(got != want)[:5])
    return t, q, want


# ---- 1. designed names: device == host, at every alignment of the bytes and of the query buffer ----
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_device_equals_host(ca, eng, name):
    data, rp = TEXTS[name]
    for lead in range(4):
        check(ca, eng, name, data, rp, lead, (lead + 1) % 4)


@pytest.mark.parametrize("name", ["tail_short", "tail_260", "tail_empty_name", "prefixes", "lengths_fq"])
def test_every_pair_of_alignments(ca, eng, name):
    data, rp = TEXTS[name]
    for lead in range(4):
        for qlead in range(4):
            check(ca, eng, name, data, rp, lead, qlead)


def test_lane_and_wave_kernel_on_both_sides(ca, eng):
    """names and queries of 259 / 260 / 261 and 1 000 bytes: found where they are equal, not where one byte or the length differs"""
    data, rp = TEXTS["lengths_fa"]
    d = name_sets.first_by_name(data, rp)
    by_len = {len(k): k for k in d}
    q = []
    for n in (259, 260, 261, 1000):
        nm = by_len[n]
        q += [nm, nm[:-1], nm + b"x", nm[:100] + name_sets.other(nm[100:101]) + nm[101:], nm[:-1] + b" ", nm[:n // 2] + b" " + nm[n // 2:]]
    t, q, want = check(ca, eng, "lane_wave", data, rp, 1, 3, q)
    assert [int(w) != NF for w in want] == [True, False, False, False, False, False] * 4


# ---- 2. tables of 1 .. 40 records, the hash cut to 0, 1, 3 bits and whole: one chain, chains that wrap, equal tags ----
@pytest.mark.parametrize("bits", [0, 1, 3, None])
def test_probe_chains(ca, bits):
    """bits 0: every name and every query on one chain with one tag; 1 and 3: a table of 2 .. 8 slots holds chains that start in
    its last slots and wrap (6 to 16 seeds per size, so that some do: a table of one record has two slots, and the record lies
    in the second for about half of the names), absent queries that meet a free slot only behind the wrap,
    absent queries whose tag is a present one's (all tags are 0)"""
    with engine_with_hash_bits(ca, bits) as e:
        for n in range(1, 41):
            for seed in range(16 if n <= 2 else 6 if n <= 8 else 1):
                data, rp = name_sets.chain(n, seed)
                check(ca, e, "chain %d %d" % (n, seed), data, rp, (n + seed) % 4, (n + 2 * seed) % 4)
        for name in ("lengths_fa", "long_prefixes", "high_bytes", "tail_260"):
            data, rp = TEXTS[name]
            check(ca, e, name, data, rp, 3, 2)


# ---- 3. how many queries a call takes ----
@pytest.fixture(scope="module")
def many(ca):
    rng = random.Random(5)
    recs = [fastx_sets.fq(b"lane%d:%d/1 c" % (i % 7, i // 3), fastx_sets.acgt(rng, 30)) for i in range(3000)]
    data, rp = name_sets.build(recs)
    present = list(name_sets.first_by_name(data, rp))
    q = [rng.choice(present) if rng.random() < 0.6 else rng.choice(present) + rng.choice([b"0", b"/", b""]) for _ in range(5000)]
    q[17] = name_sets.rand_name(rng, 400)
    q[4000] = b""
    return data, rp, q


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_query_counts(ca, eng, many, n):
    data, rp, q = many
    check(ca, eng, "many %d" % n, data, rp, 2, 1, q[:n])


def test_duplicate_queries(ca, eng, many):
    data, rp, q = many
    qq = [name_sets.name_at(data, int(rp[5]))] * 70 + [b"absent"] * 70 + q[:10] * 3
    t, qq, want = check(ca, eng, "dups", data, rp, 0, 0, qq)
    assert len(set(want[:70].tolist())) == 1 and int(want[0]) != NF and np.all(want[70:140] == NF)


# ---- 4. the table's life ----
def test_two_finds_then_another_build_then_drop(ca, eng):
    d1, r1 = TEXTS["prefixes"]
    d2, r2 = TEXTS["repeats"]
    q = name_sets.queries(d1, r1) + name_sets.queries(d2, r2)
    w1, w2 = ca.find_names(d1, r1, q), ca.find_names(d2, r2, q)
    assert not np.array_equal(w1, w2)
    big1, t1 = device_copy(d1, 1)
    big2, t2 = device_copy(d2, 2)
    eng.names_build(t1, r1)
    assert np.array_equal(eng.names_find(q), w1)
    assert np.array_equal(eng.names_find(q[::-1]), w1[::-1])
    assert len(eng.names_find([])) == 0
    eng.names_build(t2, r2)                               # the first table is gone
    del big1, t1
    assert np.array_equal(eng.names_find(q), w2)
    eng.names_drop()
    with pytest.raises(ca.CrassError) as err:
        eng.names_find(q)
    assert err.value.status == 6
    eng.names_drop()                                      # without a table: fine


def test_no_records(ca, eng):
    big, t = device_copy(b"ACGT")
    eng.names_build(t, np.asarray([4], np.uint64))        # n_reads == 0
    assert eng.names_find([b"", b"ACGT", b"a b"]).tolist() == [NF] * 3
    assert len(eng.names_find([])) == 0
    eng.names_drop()


def test_header_ids_stay_what_they_are(ca, eng):
    """crass_hip_fastx_header_ids_device before, between and after build, find and drop on one context"""
    data, rp = TEXTS["lengths_fa"]
    want = ca.fastx_header_ids(data, rp)
    big, t = device_copy(data, 3)
    q = name_sets.queries(data, rp)
    wf = want_of(ca, "lengths_fa", data, rp, q)

    def ids():
        got, n_rep = eng.device_header_ids(t, rp, install=False)
        assert np.array_equal(got, want) and n_rep == int(np.count_nonzero(want != np.arange(len(want), dtype=np.uint64)))

    ids()
    eng.names_build(t, rp)
    ids()
    assert np.array_equal(eng.names_find(q), wf)          # (the header ids' scratch was not the table)
    ids()
    eng.names_drop()
    ids()


# ---- 5. the files route ----
def test_files_route(ca):
    rng = random.Random(9)
    f0 = b"".join(fastx_sets.fq(b"pair%d/1 first file" % i, fastx_sets.acgt(rng, 40)) for i in range(300))
    f1 = b"".join(fastx_sets.fq(b"pair%d/%d second" % (i, 1 + i % 2), fastx_sets.acgt(rng, 40)) for i in range(299, -1, -1))
    files = [f0, bgzf_sets.bgzf(f1, block=4000)]
    with ca.SearchEngine() as e:
        with pytest.raises(ca.CrassError) as err:
            e.names_build(None, None)                     # no files loaded
        assert err.value.status == 6
        lay = e.load_fastx_files(files)
        host = ca.engine.fastx_files_scan_host(files)
        assert np.array_equal(lay.rec_pos, host.rec_pos) and lay.n_reads == 600
        arena = f0 + b"\n" + f1 + b"\n"
        assert int(lay.rec_pos[-1]) == len(arena) - 1
        q = [b"pair%d/%d" % (i, k) for i in range(0, 300, 7) for k in (1, 2, 3)] + [b"pair", b""]
        want = ca.find_names(arena, lay.rec_pos, q)
        assert np.count_nonzero(want >= 300) > 10 and np.count_nonzero(want < 300) > 10 and np.count_nonzero(want == NF) > 10
        e.names_build(None, None)
        assert np.array_equal(e.names_find(q), want)      # indices over both files
        ids, _ = e.device_header_ids(e.resident_fastx()[0], np.append(lay.rec_pos[:-1], np.uint64(e.resident_fastx()[1])), install=False)
        names = [name_sets.name_at(arena, int(p)) for p in lay.rec_pos[:-1]]
        assert np.array_equal(e.names_find(names), ids)
        e.load_fastx_files([f0])                          # a later load drops the table
        with pytest.raises(ca.CrassError) as err:
            e.names_find(q)
        assert err.value.status == 6
        lay1 = e.load_fastx_files([f0])
        e.names_build(None, None)
        assert np.array_equal(e.names_find(q), ca.find_names(f0 + b"\n", lay1.rec_pos, q))
    # a table on the caller's own bytes outlives a load
    data, rp = TEXTS["prefixes"]
    qq = name_sets.queries(data, rp)
    with ca.SearchEngine() as e:
        big, t = device_copy(data)
        e.names_build(t, rp)
        e.load_fastx_files([f0])
        assert np.array_equal(e.names_find(qq), ca.find_names(data, rp, qq))


# ---- 6. errors: the documented status, the table before as it was ----
def test_errors(ca):
    lib = ca.load()
    build, find = lib.crass_hip_fastx_names_build_device, lib.crass_hip_fastx_names_find
    data, rp = TEXTS["repeats"]
    n = len(rp) - 1
    big, t = device_copy(data)
    ptr, nb = int(t.data_ptr()), len(data)
    q = name_sets.queries(data, rp)
    want = ca.find_names(data, rp, q)
    chars, off = name_sets.concat(q)
    out = np.full(len(q), 12345, np.uint64)
    with ca.SearchEngine() as e:
        assert find(e.h, chars.ctypes.data, off.ctypes.data, len(q), out.ctypes.data) == 6      # no table
        bad = rp.copy()
        bad[n // 2] = nb                                  # a record position at the input's end
        assert build(e.h, ptr, nb, bad.ctypes.data, n) == 1
        assert find(e.h, chars.ctypes.data, off.ctypes.data, len(q), out.ctypes.data) == 6      # ... and no table is kept
        assert np.all(out == 12345)
        assert build(e.h, ptr, nb, rp.ctypes.data, n) == 0
        assert build(e.h, None, nb, rp.ctypes.data, n) == 1 and build(e.h, ptr, nb, None, n) == 1
        assert build(e.h, ptr, nb, rp.ctypes.data, 2 ** 32 - 1) == 2
        bad[n // 2] = 2 ** 63
        assert build(e.h, ptr, nb, bad.ctypes.data, n) == 1
        assert find(e.h, None, off.ctypes.data, len(q), out.ctypes.data) == 1
        assert find(e.h, chars.ctypes.data, None, len(q), out.ctypes.data) == 1
        assert find(e.h, chars.ctypes.data, off.ctypes.data, len(q), None) == 1
        down = off.copy()
        down[3] = down[4] + 1
        assert find(e.h, chars.ctypes.data, down.ctypes.data, len(q), out.ctypes.data) == 1
        assert np.all(out == 12345)
        assert find(e.h, None, None, 0, None) == 0                                             # no queries: fine
        # the table of the one accepted build answers as before
        assert find(e.h, chars.ctypes.data, off.ctypes.data, len(q), out.ctypes.data) == 0 and np.array_equal(out, want)
        assert lib.crass_hip_fastx_names_drop(e.h) == 0 and lib.crass_hip_fastx_names_drop(e.h) == 0
        assert find(e.h, chars.ctypes.data, off.ctypes.data, len(q), out.ctypes.data) == 6
        assert e.counters()["n_reads"] == 0


def test_times_are_reported_when_asked_for(ca, eng, many):
    data, rp, q = many
    big, t = device_copy(data)
    eng.names_build(t, rp)
    eng.names_find(q)
    assert eng.last_names_ms() == (0.0, 0.0)
    eng.set_stage_timing(1)
    try:
        eng.names_build(t, rp)
        eng.names_find(q)
        b, f = eng.last_names_ms()
        assert b > 0 and f > 0
    finally:
        eng.set_stage_timing(0)
        eng.names_drop()
