"""Wrapped FASTQ parsed on the device (crass_hip_set_fastq_class, fastx_wrapped.hip) against the host rule
(crass_fastx_scan_host_class) and against the same reads loaded as four-line FASTQ: every designed input of
tests/wrapped_sets.py through load_fastx_bytes and through attach_device_fastx at three address offsets, every designed decline,
class 0 declining as before, several files as one set, the BGZF and gzip routes, the same candidates and recruits, and the
scratch given back.  Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

from tests import bgzf_sets, fastx_sets, gzip_sets, wrapped_sets

pytestmark = pytest.mark.gpu

T = 4096
PAD = 2
ARRAYS = ("packed", "word_off", "lengths", "exc_read", "exc_off", "exc_bytes", "header_id")
SCALARS = ("n_reads", "stride_words", "uniform_len", "n_exceptions", "read_index_base")
DESIGNED = wrapped_sets.designed(T)
DECLINES = wrapped_sets.declines(T)


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    assert crass_amd.load().crass_hip_fastx_tile_bytes() == T
    return crass_amd


@pytest.fixture(scope="module")
def eng(ca):
    """class 1"""
    with ca.SearchEngine() as e:
        e.set_fastq_class(1)
        yield e


@pytest.fixture(scope="module")
def eng4(ca):
    """class 0, the default"""
    with ca.SearchEngine() as e:
        yield e


_refs = {}


def reference(ca, eng4, name):
    """the host rule's layout, and the packed set of the same reads loaded as four-line FASTQ by the class-0 context: once per input"""
    if name not in _refs:
        data = DESIGNED[name]
        host = ca.fastx_scan_host(data, fastq_class=1)
        assert host.accepted, name
        flat = wrapped_sets.unwrapped(data)
        lay = eng4.load_fastx_bytes(flat, pad_uniform=PAD)
        assert lay.n_reads == host.n_reads and np.array_equal(lay.seq_off, host.seq_off), name
        res = eng4.packed()
        _refs[name] = (host, res.arrays())
        res.close()
    return _refs[name]


def assert_same_set(got, want, what):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert np.array_equal(got[k], want[k]), (what, k)


def check_resident(eng, lay, ref, name, what):
    host, want = ref
    assert lay.accepted and (lay.n_reads, lay.format, lay.max_len, lay.decline_pos) == (host.n_reads, b"@", host.max_len, 0), what
    assert np.array_equal(lay.rec_pos, host.rec_pos) and np.array_equal(lay.seq_off, host.seq_off), what
    res = eng.packed()
    assert_same_set(res.arrays(), want, what)
    res.close()
    assert eng.last_scan_classes() == ((1, 0) if name in wrapped_sets.FOUR_LINE else (0, 1)), what


def device_copy(data, lead=0):
    import torch
    big = torch.full((len(data) + lead + 64,), 0x40, dtype=torch.uint8, device="cuda")      # ('@' around the input: nothing outside it may be read)
    t = big[lead:lead + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    assert t.data_ptr() % 16 == lead % 16
    return big, t


def attach(eng, data, lead):
    big, t = device_copy(data, lead)
    try:
        return eng.attach_device_fastx(t, pad_uniform=PAD)
    finally:
        del t, big


# ---- 1. accepted inputs ----
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_inputs_give_the_unwrapped_set(ca, eng, eng4, name):
    data = DESIGNED[name]
    ref = reference(ca, eng4, name)
    lay = eng.load_fastx_bytes(data, pad_uniform=PAD)
    check_resident(eng, lay, ref, name, name + " load_fastx_bytes")
    for lead in (0, 1, 15):
        lay = attach(eng, data, lead)
        check_resident(eng, lay, ref, name, "%s attach_device_fastx lead %d" % (name, lead))


@pytest.mark.parametrize("last", ["one_line", "two_lines"])
def test_more_lines_than_one_step_of_the_rank_scan(ca, eng, eng4, last):
    """65 537 four-line records of one base and a blank line behind them: more than 256 * 1024 lines, so the one block over the
    rank scan's tiles takes a second step for both of its sums, with the carries of the first in front.  The layout is the host
    rule's, the packed set that of the same reads as four-line FASTQ; then with the last record's sequence over two lines"""
    n = 65537
    tail = b"@r\nG\n+\nI\n" if last == "one_line" else b"@r\nG\nT\n+\nIJ\n"
    data = b"@r\nA\n+\nI\n" * (n - 1) + tail + b"\n"
    assert data.count(b"\n") > 256 * 1024
    host = ca.fastx_scan_host(data, fastq_class=1)
    assert host.accepted and host.n_reads == n and host.max_len == (1 if last == "one_line" else 2)
    assert not ca.fastx_scan_host(data).accepted         # (the blank line: the four-line scan leaves it to the wrapped one)
    eng4.load_fastx_bytes(b"@r\nA\n+\nI\n" * (n - 1) + (tail if last == "one_line" else b"@r\nGT\n+\nIJ\n"), pad_uniform=PAD)
    want = eng4.packed()
    lay = eng.load_fastx_bytes(data, pad_uniform=PAD)
    assert eng.last_scan_classes() == (0, 1)
    assert lay.accepted and (lay.n_reads, lay.format, lay.max_len, lay.decline_pos) == (n, b"@", host.max_len, 0)
    assert np.array_equal(lay.rec_pos, host.rec_pos) and np.array_equal(lay.seq_off, host.seq_off)
    got = eng.packed()
    assert_same_set(got.arrays(), want.arrays(), last)
    got.close()
    want.close()


# ---- 2. class 0 declines as before; class 1 declines with the host rule's verdict ----
@pytest.mark.parametrize("name", sorted(n for n in DESIGNED if n not in wrapped_sets.FOUR_LINE and not n.startswith("records_")) + ["records_65"])
def test_class_zero_declines_as_before(ca, eng4, name):
    data = DESIGNED[name]
    host = ca.fastx_scan_host(data)
    assert not host.accepted
    for route in ("host", "device"):
        with pytest.raises(ca.FastxDeclined) as e:
            eng4.load_fastx_bytes(data) if route == "host" else attach(eng4, data, 0)
        lay = e.value.layout
        assert e.value.status == 2 and (lay.decline_reason, lay.decline_pos, lay.n_reads) == (host.decline_reason, host.decline_pos, 0), (name, route)
        assert eng4.last_scan_classes() == (1, 0)


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_designed_declines_get_the_host_verdict(ca, eng, name):
    import torch
    data, reason, pos = DECLINES[name]
    host = ca.fastx_scan_host(data, fastq_class=1)
    assert (host.decline_reason, host.decline_pos) == (reason, pos)
    for route in ("host", "device"):
        eng.load_fastx_bytes(DESIGNED["wrap7"])          # something resident, so that the decline has something to take away
        with pytest.raises(ca.FastxDeclined) as e:
            if route == "host":
                eng.load_fastx_bytes(data)
            elif len(data):
                attach(eng, data, 3)
            else:
                eng.attach_device_fastx(torch.zeros(0, dtype=torch.uint8, device="cuda"))
        lay = e.value.layout
        assert e.value.status == 2 and (lay.decline_reason, lay.decline_pos, lay.n_reads) == (reason, pos, 0), (name, route, lay.decline_reason, lay.decline_pos)
        assert len(lay.rec_pos) == 0 and eng.counters()["n_reads"] == 0
        with pytest.raises(ca.CrassError) as e:
            eng.seed_scan()
        assert e.value.status == 6


def test_the_four_line_scans_final_declines_stay(ca, eng):
    """FASTA is no business of the class, and a four-line decline for a read too long is not taken up"""
    for name, (data, reason, pos) in fastx_sets.irregular(T).items():
        if data[:1] == b">":
            with pytest.raises(ca.FastxDeclined) as e:
                eng.load_fastx_bytes(data)
            assert (e.value.layout.decline_reason, e.value.layout.decline_pos) == (reason, pos), name
    too_long = b"@a\nACGT\n+\nIIII\n@long\n" + b"ACGT\n" * 15001 + b"+\n" + b"IIII\n" * 15001
    with pytest.raises(ca.FastxDeclined) as e:
        eng.load_fastx_bytes(too_long)
    assert (e.value.layout.decline_reason, e.value.layout.decline_pos) == (11, 15)
    lib = ca.load()
    assert lib.crass_hip_set_fastq_class(eng.h, 2) == 1 and lib.crass_hip_set_fastq_class(None, 1) == 1
    assert lib.crass_hip_last_scan_classes(eng.h, None) == 1


def test_seeded_sweep_agrees_with_the_host_rule(ca, eng):
    """300 files drawn from the class's grammar and 300 one-byte mutations of such files: the device's verdict and layout are
    the host rule's on every one"""
    import random
    rng = random.Random(20261023)
    accepted = 0
    for k in range(600):
        data = wrapped_sets.generate(rng)
        if k % 2:
            data = wrapped_sets.mutate(rng, data)
        host = ca.fastx_scan_host(data, fastq_class=1)
        try:
            lay = eng.load_fastx_bytes(data, pad_uniform=PAD)
        except ca.FastxDeclined as e:
            lay = e.layout
        assert (lay.accepted, lay.decline_reason, lay.decline_pos, lay.n_reads, lay.max_len) == \
            (host.accepted, host.decline_reason, host.decline_pos, host.n_reads, host.max_len), (k, data, lay.decline_reason, lay.decline_pos)
        assert np.array_equal(lay.rec_pos, host.rec_pos) and np.array_equal(lay.seq_off, host.seq_off), (k, data)
        accepted += lay.accepted
    assert accepted >= 300


# ---- 3. several files, BGZF, gzip ----
def test_files_as_one_set(ca, eng, eng4):
    files = [DESIGNED["four_line"], DESIGNED["void_lines"], fastx_sets.regular()["wrap60"]]
    host = ca.fastx_files_scan_host(files, fastq_class=1)
    assert host.accepted
    lay = eng.load_fastx_files(files, pad_uniform=PAD)
    assert eng.last_scan_classes() == (2, 1)
    assert lay.accepted and lay.n_reads == host.n_reads and lay.max_len == host.max_len
    for k in ("rec_pos", "seq_off", "file_read_base", "file_byte_base"):
        assert np.array_equal(getattr(lay, k), getattr(host, k)), k
    got = eng.packed()
    flat = [files[0], wrapped_sets.unwrapped(files[1]), files[2]]
    eng4.load_fastx_files(flat, pad_uniform=PAD)
    want = eng4.packed()
    assert_same_set(got.arrays(), want.arrays(), "three files")
    got.close()
    want.close()
    with pytest.raises(ca.FastxFilesDeclined) as e:
        eng4.load_fastx_files(files, pad_uniform=PAD)
    four = ca.fastx_files_scan_host(files)
    assert (e.value.layout.decline_file, e.value.layout.decline_reason, e.value.layout.decline_pos) == (1, four.decline_reason, four.decline_pos)
    bad = files[:2] + [DECLINES["qual_passes_third_tile"][0]]
    with pytest.raises(ca.FastxFilesDeclined) as e:
        eng.load_fastx_files(bad, pad_uniform=PAD)
    assert (e.value.layout.decline_file, e.value.layout.decline_reason, e.value.layout.decline_pos) == (2,) + DECLINES["qual_passes_third_tile"][1:]


@pytest.mark.parametrize("name", ["void_lines", "read_9000_wrap60"])
def test_compressed_routes(ca, eng, eng4, name):
    data = DESIGNED[name]
    ref = reference(ca, eng4, name)
    lay = eng.load_fastx_bgzf(bgzf_sets.bgzf(data, block=3000), pad_uniform=PAD)
    check_resident(eng, lay, ref, name, name + " load_fastx_bgzf")
    lay = eng.load_fastx_gzip(gzip_sets.gz(data), pad_uniform=PAD)
    check_resident(eng, lay, ref, name, name + " load_fastx_gzip")
    half = data.index(b"\n", len(data) // 2) + 1
    lay = eng.load_fastx_gzip_members(gzip_sets.gz(data[:half]) + gzip_sets.gz(data[half:]), pad_uniform=PAD)
    check_resident(eng, lay, ref, name, name + " load_fastx_gzip_members")
    host = ca.fastx_scan_host(data, fastq_class=1)
    eng.set_gzip_on_device(True)
    try:
        for packed_file in (bgzf_sets.bgzf(data, block=3000), gzip_sets.gz(data)):
            lay = eng.load_fastx_files([packed_file], pad_uniform=PAD)
            assert lay.n_reads == host.n_reads and np.array_equal(lay.rec_pos, host.rec_pos) and np.array_equal(lay.seq_off, host.seq_off)
            assert eng.last_scan_classes() == (0, 1)
    finally:
        eng.set_gzip_on_device(False)


# ---- 4. the same answers through the path ----
def assert_same_fields(a, b, what):
    keys = sorted(k for k in vars(a) if not k.startswith("_"))
    assert type(a) is type(b) and keys == sorted(k for k in vars(b) if not k.startswith("_")) and keys, what
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)
        else:
            assert x == y, (what, k)


def test_same_candidates_and_recruits(ca, eng, eng4):
    n, L = 1500, 150
    words = ca.synth_packed(ca.synth_spec(read_len=L, seed=11, crispr_per_million=100000), 0, n)
    asc = ca.unpack_ascii(words, (L + 15) // 16, L, n)
    seqs = [asc[i * L:(i + 1) * L].tobytes() for i in range(n)]
    data = b"".join(wrapped_sets.wfq(b"read%d c" % i, s, w=60, after=(b"",) if i % 7 == 0 else ()) for i, s in enumerate(seqs))
    eng.load_fastx_bytes(data, pad_uniform=PAD)
    assert eng.last_scan_classes() == (0, 1)
    eng4.load_fastx_bytes(wrapped_sets.unwrapped(data), pad_uniform=PAD)
    ra = (eng.seed_scan(), eng.merge(), eng.recruit())
    rb = (eng4.seed_scan(), eng4.merge(), eng4.recruit())
    for x, y, part in zip(ra, rb, ("candidates", "merge", "recruits")):
        assert_same_fields(x, y, part)
    assert ra[0].n >= 20 and ra[1].n_patterns > 0
    found = np.concatenate([ra[0].read_idx, ra[2].read_idx])
    text = eng.fetch_text(found)
    assert [text[k] for k in range(len(found))] == [seqs[int(r)] for r in found]


# ---- 5. the scratch goes back ----
def test_ingest_scratch_is_given_back(ca):
    lib = ca.load()
    lib.crassi_dev_bytes_live.restype = C.c_uint64
    lib.crassi_dev_bytes_live.argtypes = []
    live = lambda: int(lib.crassi_dev_bytes_live())
    data = DESIGNED["records_1025"]
    with ca.SearchEngine() as e:
        e.set_fastq_class(1)
        e.load_fastx_bytes(wrapped_sets.unwrapped(data), pad_uniform=PAD)
        want = live()
        after = []
        for _ in range(3):
            e.load_fastx_bytes(data, pad_uniform=PAD)
            after.append(live())
        assert after == [want] * 3, (after, want)
        attach(e, data, 5)
        assert live() == want
        for _ in range(2):
            with pytest.raises(ca.FastxDeclined):
                e.load_fastx_bytes(DECLINES["qual_passes_third_tile"][0], pad_uniform=PAD)
            assert live() <= want
        with pytest.raises(ca.FastxFilesDeclined):
            e.load_fastx_files([data, DECLINES["qual_del_last"][0]], pad_uniform=PAD)
        assert live() <= want
        e.load_fastx_bytes(data, pad_uniform=PAD)
        assert live() == want
