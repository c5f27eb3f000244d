"""Header ids and header lines from FASTA / FASTQ bytes that live on the device (crass_hip_fastx_header_ids_device,
crass_hip_fetch_header_lines_device, fastx_hid.hip, fastx_lines.hip) against the host: crass_fastx_header_ids on the same bytes, the lines
sliced from the bytes in Python, the names crass_read_fastx (kseq) cuts, and the same answers through seed scan, merge and
recruit.  Every comparison is exact equality."""
import os

import numpy as np
import pytest

from tests import fastx_sets, header_sets

pytestmark = pytest.mark.gpu

T = 4096
REGULAR = dict(fastx_sets.regular(), **fastx_sets.tile_edge(T))
DESIGNED = header_sets.designed()
INPUTS = dict(REGULAR, **DESIGNED)
LEADS = (0, 1, 7, 15)


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


_refs = {}


def reference(ca, name):
    """the host's layout, header ids and header lines of an input: once per input"""
    if name not in _refs:
        data = INPUTS[name]
        lay = ca.fastx_scan_host(data)
        assert lay.accepted, name
        hid = ca.fastx_header_ids(data, lay.rec_pos)
        _refs[name] = (lay, hid, header_sets.header_lines(data, lay.rec_pos))
    return _refs[name]


def device_copy(data, lead=0):
    """the bytes in a fresh device tensor that starts `lead` bytes behind an aligned allocation, '>' all around them"""
    import torch
    big = torch.full((len(data) + lead + 64,), 0x3E, dtype=torch.uint8, device="cuda")
    t = big[lead:lead + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    assert t.data_ptr() % 16 == lead % 16
    return big, t


def engine_with_hash_bits(ca, bits):
    old = os.environ.pop("CRASS_HID_TEST_HASH_BITS", None)
    os.environ["CRASS_HID_TEST_HASH_BITS"] = str(bits)
    try:
        return ca.SearchEngine()                          # (the switch is read when the context is created)
    finally:
        os.environ.pop("CRASS_HID_TEST_HASH_BITS", None)
        if old is not None:
            os.environ["CRASS_HID_TEST_HASH_BITS"] = old


def check_ids(ca, e, name, lead, install):
    data = INPUTS[name]
    lay_h, want, _ = reference(ca, name)
    big, t = device_copy(data, lead)
    what = "%s lead %d" % (name, lead)
    if install:
        lay = e.attach_device_fastx(t, pad_uniform=2)
        assert np.array_equal(lay.rec_pos, lay_h.rec_pos), what
    else:
        lay = lay_h
    ids, n_rep = e.device_header_ids(t, lay, install=install)
    assert ids.dtype == np.uint64 and np.array_equal(ids, want), (what, np.flatnonzero(ids != want)[:5])
    assert n_rep == int(np.count_nonzero(want != np.arange(len(want), dtype=np.uint64))), what
    if install:
        res = e.packed()
        got = res.arrays()["header_id"]
        assert got is not None and np.array_equal(got, want), what
        res.close()


# ---- 1. ids equal the host's, returned and installed ----
@pytest.mark.parametrize("name", sorted(REGULAR))
def test_ids_equal_the_hosts(ca, eng, name):
    check_ids(ca, eng, name, 0, True)


# ---- 2. designed names, at four alignments of the bytes ----
def name_of(line):
    for i, c in enumerate(line):
        if c == 32 or 9 <= c <= 13:
            return line[:i]
    return line


def test_the_designed_input_is_what_it_says(ca):
    lay, hid, lines = reference(ca, "designed")
    assert lay.n_reads <= 200
    names = [name_of(ln) for ln in lines]
    long_ones = [r for r, nm in enumerate(names) if len(nm) == header_sets.LONG]
    assert len(long_ones) == 5 and [int(hid[r]) for r in long_ones] == [long_ones[0], long_ones[0], long_ones[2], long_ones[2], long_ones[0]]
    assert long_ones[-1] == lay.n_reads - 1 and int(lay.rec_pos[-1]) == int(lay.rec_pos[-2]) + 1 + header_sets.LONG      # it ends with the input
    assert names.count(b"") == 4
    same = [r for r, ln in enumerate(lines) if ln == b"same-name-everywhere/1"]
    assert sorted(int(lay.rec_pos[r]) % 16 for r in same) == list(range(16)) and all(int(hid[r]) == same[0] for r in same)
    assert len(set(int(h) for h in hid)) < lay.n_reads and len(set(int(h) for h in hid)) > 50


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_names(ca, eng, name, lead):
    check_ids(ca, eng, name, lead, True)


@pytest.mark.parametrize("name", ["one_header", "header_last_nonl", "T_plus_1_name_in_next_tile", "odd_headers", "dup_names", "fq_crlf"])
def test_regular_names_at_odd_addresses(ca, eng, name):
    for lead in LEADS[1:]:
        check_ids(ca, eng, name, lead, False)


# ---- 3. collisions: the hash cut to 0, 2 and 33 bits; the byte comparison decides ----
@pytest.mark.parametrize("bits", [0, 2, 33])
def test_collisions(ca, bits):
    with engine_with_hash_bits(ca, bits) as e:
        for name in sorted(INPUTS):
            check_ids(ca, e, name, 0, False)
        for lead in LEADS[1:]:
            check_ids(ca, e, "designed", lead, False)
        check_ids(ca, e, "dup_names", 0, True)
        check_ids(ca, e, "designed", 7, True)


# ---- 4. the same answers through the path ----
def run_path(e):
    return e.seed_scan(), e.merge(), e.recruit()


def assert_same_fields(a, b, what):
    assert type(a) is type(b)
    keys = sorted(k for k in vars(a) if not k.startswith("_"))
    assert keys == sorted(k for k in vars(b) if not k.startswith("_")) and keys, what
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)
        else:
            assert x == y, (what, k)


def synth_mates(ca):
    """6 000 synthetic 150-base reads, one in ten with a planted array, as a FASTA wrapped at 60 columns; reads 2 k and 2 k + 1
    share a name"""
    n, L = 6000, 150
    words = ca.synth_packed(ca.synth_spec(read_len=L, seed=11, crispr_per_million=100000), 0, n)
    asc = ca.unpack_ascii(words, (L + 15) // 16, L, n)
    seqs = [asc[i * L:(i + 1) * L].tobytes() for i in range(n)]
    return seqs, b"".join(fastx_sets.fa(b"read%d/x comment" % (i // 2), s, 60) for i, s in enumerate(seqs))


def test_same_answers_through_the_path(ca):
    seqs, data = synth_mates(ca)
    big, t = device_copy(data, 3)
    with ca.SearchEngine() as a, ca.SearchEngine() as b:
        lay = a.attach_device_fastx(t, pad_uniform=2)
        plain = run_path(a)
        ids, n_rep = a.device_header_ids(t, lay, install=True)
        cnt = a.counters()
        assert cnt["n_reads"] == len(seqs) and cnt["n_pass1_found"] == 0      # the reads stay, the results are gone
        with pytest.raises(ca.CrassError) as e:
            a.recruits()
        assert e.value.status == 6
        lay_b = b.attach_device_fastx(t, pad_uniform=2)
        hid = ca.fastx_header_ids(data, lay_b.rec_pos)
        assert np.array_equal(hid, (np.arange(len(seqs), dtype=np.uint64) // 2) * 2)
        assert np.array_equal(ids, hid) and n_rep == len(seqs) // 2
        b.set_header_ids(hid)
        ra, rb = run_path(a), run_path(b)
        for x, y, part in zip(ra, rb, ("candidates", "merge", "recruits")):
            assert_same_fields(x, y, part)
        for k in ("n_reads", "n_exceptions", "n_pass1_found", "n_pass2_found", "n_patterns", "bytes_reads_device", "used_fast_filter"):
            assert a.counters()[k] == b.counters()[k], k
        assert ra[0].n >= 100 and ra[1].n_patterns > 0 and 0 < ra[2].n < plain[2].n      # mates of pass-1 hits stay out of pass 2


# ---- 5. header lines ----
_names = {}


def kseq_name_lengths(ca, tmp_path_factory, name):
    if name not in _names:
        p = tmp_path_factory.mktemp("hl") / "in.fx"
        p.write_bytes(INPUTS[name])
        f = ca.FastxFile(str(p))
        _names[name] = np.diff(f.name_off.astype(np.int64))
    return _names[name]


def index_lists(n):
    rev = list(range(n - 1, -1, -3))
    return [list(range(n)), rev, [n // 2, 0, n // 2, n - 1, n // 2], []]


def check_lines(ca, e, tmp_path_factory, name, lead):
    import torch
    data = INPUTS[name]
    lay, _, lines = reference(ca, name)
    klen = kseq_name_lengths(ca, tmp_path_factory, name)
    assert len(klen) == lay.n_reads
    big, t = device_copy(data, lead)
    for idx in index_lists(lay.n_reads):
        what = "%s lead %d, %d records" % (name, lead, len(idx))
        want = [lines[r] for r in idx]
        want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
        chars, off, name_len = e.fetch_header_lines(t, lay, idx)
        assert off.dtype == np.uint64 and np.array_equal(off, want_off), what
        assert chars.tobytes() == b"".join(want), what
        assert name_len.dtype == np.uint32 and np.array_equal(name_len, np.asarray([klen[r] for r in idx], dtype=np.uint32)), what
        # into the caller's device buffer, guard bytes on both sides
        total, G = int(want_off[-1]), 37
        buf = torch.full((total + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        none, off2, name_len2 = e.fetch_header_lines(t, lay, idx, out=buf[G:G + total])
        got = buf.cpu().numpy()
        assert none is None and np.array_equal(off2, want_off) and np.array_equal(name_len2, name_len), what
        assert got[G:G + total].tobytes() == b"".join(want), what
        assert np.all(got[:G] == 0xA5) and np.all(got[G + total:] == 0xA5), what


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_header_lines(ca, eng, tmp_path_factory, name):
    check_lines(ca, eng, tmp_path_factory, name, 0)


@pytest.mark.parametrize("name", ["designed", "tail_dupe", "crlf", "one_header", "T_plus_1_name_in_next_tile", "fq_four_tiles"])
def test_header_lines_at_odd_addresses(ca, eng, tmp_path_factory, name):
    for lead in LEADS[1:]:
        check_lines(ca, eng, tmp_path_factory, name, lead)


def test_header_lines_buffer_too_small(ca, eng):
    import torch
    data = INPUTS["dup_names"]
    lay, _, lines = reference(ca, "dup_names")
    big, t = device_copy(data)
    buf = torch.full((len(lines[0]) + len(lines[1]) - 1,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(ca.CrassError) as e:
        eng.fetch_header_lines(t, lay, [0, 1], out=buf)
    assert e.value.status == 8 and list(e.value.offsets) == [0, len(lines[0]), len(lines[0]) + len(lines[1])]
    assert bool((buf == 0xA5).all())


# ---- 6. errors: the documented status, nothing installed, the resident set as it was ----
def test_errors(ca):
    import torch
    lib = ca.load()
    data = INPUTS["dup_names"]
    lay_h, want, _ = reference(ca, "dup_names")
    big, t = device_copy(data)
    ptr, nb = int(t.data_ptr()), len(data)
    rp = np.ascontiguousarray(lay_h.rec_pos)
    n = lay_h.n_reads
    out = np.full(n, 12345, np.uint64)
    ids_fn, lines_fn = lib.crass_hip_fastx_header_ids_device, lib.crass_hip_fetch_header_lines_device
    import ctypes as C
    from crass_amd import _abi
    idx = np.arange(n, dtype=np.uint64)
    with ca.SearchEngine() as e:
        # no reads resident: installing is a state error, computing alone is fine
        assert ids_fn(e.h, ptr, nb, rp.ctypes.data, n, out.ctypes.data, 1, None) == 6
        assert np.all(out == 12345)
        assert ids_fn(e.h, ptr, nb, rp.ctypes.data, n, out.ctypes.data, 0, None) == 0 and np.array_equal(out, want)
        assert e.counters()["n_reads"] == 0
        with pytest.raises(ca.CrassError) as err:
            e.seed_scan()
        assert err.value.status == 6
        lay = e.attach_device_fastx(t, pad_uniform=2)
        marker = np.zeros(n, np.uint64)                   # ids of our own, to see that a failed call leaves them
        assert not np.array_equal(marker, want)
        e.set_header_ids(marker)
        before = e.packed()
        arrays = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in before.arrays().items()}
        assert np.array_equal(arrays["header_id"], marker)
        before.close()

        def untouched(what):
            res = e.packed()
            got = res.arrays()
            for k, v in arrays.items():
                if isinstance(v, np.ndarray):
                    assert np.array_equal(got[k], v), (what, k)
                else:
                    assert got[k] == v, (what, k)
            res.close()
            assert e.counters()["n_reads"] == n, what

        out[:] = 12345
        rep = C.c_uint64(777)
        assert ids_fn(None, ptr, nb, rp.ctypes.data, n, out.ctypes.data, 1, None) == 1                  # NULL context
        assert ids_fn(e.h, None, nb, rp.ctypes.data, n, out.ctypes.data, 1, None) == 1                  # NULL bytes
        assert ids_fn(e.h, ptr, nb, None, n, out.ctypes.data, 1, None) == 1                             # NULL rec_pos
        assert ids_fn(e.h, ptr, nb, rp.ctypes.data, n - 1, out.ctypes.data, 1, None) == 1               # not the resident set's count
        assert ids_fn(e.h, ptr, nb, rp.ctypes.data, 2 ** 32 - 1, out.ctypes.data, 0, None) == 2         # beyond a slot's index
        bad = rp.copy()
        bad[n // 2] = nb                                  # a record position at the input's end
        assert ids_fn(e.h, ptr, nb, bad.ctypes.data, n, out.ctypes.data, 1, C.byref(rep)) == 1
        bad[n // 2] = 2 ** 63
        assert ids_fn(e.h, ptr, nb, bad.ctypes.data, n, out.ctypes.data, 0, None) == 1
        assert np.all(out == 12345)
        untouched("header ids")
        assert ids_fn(e.h, None, 0, None, 0, None, 0, None) == 0                                        # no records: fine

        v = _abi.Text()
        nl = np.full(n, 999, np.uint32)
        assert lines_fn(None, ptr, nb, rp.ctypes.data, n, idx.ctypes.data, n, C.byref(v), nl.ctypes.data) == 1
        assert lines_fn(e.h, ptr, nb, rp.ctypes.data, n, idx.ctypes.data, n, None, nl.ctypes.data) == 1
        assert lines_fn(e.h, ptr, nb, rp.ctypes.data, n, None, n, C.byref(v), nl.ctypes.data) == 1
        assert lines_fn(e.h, None, nb, rp.ctypes.data, n, idx.ctypes.data, n, C.byref(v), nl.ctypes.data) == 1
        far = idx.copy()
        far[3] = n                                        # an index out of range
        assert lines_fn(e.h, ptr, nb, rp.ctypes.data, n, far.ctypes.data, n, C.byref(v), nl.ctypes.data) == 1
        assert lines_fn(e.h, ptr, nb, bad.ctypes.data, n, idx.ctypes.data, n, C.byref(v), nl.ctypes.data) == 1
        assert lines_fn(e.h, ptr, nb, rp.ctypes.data, 2 ** 32 - 1, idx.ctypes.data, n, C.byref(v), nl.ctypes.data) == 2
        assert np.all(nl == 999)
        untouched("header lines")
        # ... and the context takes the next regular call
        ids, n_rep = e.device_header_ids(t, lay, install=True)
        assert np.array_equal(ids, want)
        res = e.packed()
        assert np.array_equal(res.arrays()["header_id"], want)
        res.close()


def test_times_are_reported_when_asked_for(ca, eng):
    data = INPUTS["uniform150"]
    lay, want, _ = reference(ca, "uniform150")
    big, t = device_copy(data)
    eng.device_header_ids(t, lay, install=False)
    assert eng.last_header_ids_ms() == (0.0, 0.0, 0.0)
    eng.set_stage_timing(1)
    try:
        eng.device_header_ids(t, lay, install=False)
        whole, insert, lookup = eng.last_header_ids_ms()
        assert insert > 0 and lookup > 0 and whole >= insert
    finally:
        eng.set_stage_timing(0)
