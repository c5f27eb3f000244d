"""FASTA / FASTQ bytes parsed on the device (crass_hip_load_fastx_bytes / crass_hip_attach_device_fastx, fastx_scan.hip)
against the host route (crass_read_fastx + crass_pack_reads + crass_hip_load_reads) and the host restatement of the scan
(crass_fastx_scan_host): the resident set bit for bit, the layout, the counters, the verdict on declined inputs, and the same
answers through seed scan, merge and recruit.  Every comparison is exact equality."""
import os

import numpy as np
import pytest

from tests import fastx_sets

pytestmark = pytest.mark.gpu

T = 4096
ARRAYS = ("packed", "word_off", "lengths", "exc_read", "exc_off", "exc_bytes", "header_id")
SCALARS = ("n_reads", "stride_words", "uniform_len", "n_exceptions", "read_index_base")
REGULAR = fastx_sets.regular()
EDGE = fastx_sets.tile_edge(T)
IRREGULAR = fastx_sets.irregular(T)
INPUTS = dict(REGULAR, **EDGE)


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
    with ca.SearchEngine() as e:
        yield e


_refs = {}


def reference(ca, tmp_path_factory, name, data):
    """crass_read_fastx on the bytes, its text packed by crass_pack_reads (pad 0, 1, 2), and the host scan's layout: once per input"""
    if name not in _refs:
        p = tmp_path_factory.mktemp("fx") / "in.fx"
        p.write_bytes(data)
        f = ca.FastxFile(str(p))
        want = {}
        for pad in (0, 1, 2):
            pk = ca.PackedReads((f.seq, f.seq_off), pad_uniform=pad)
            want[pad] = ca.packed_arrays(pk.reads)
            pk.close()
        _refs[name] = (f, want, ca.fastx_scan_host(data))
    return _refs[name]


def assert_same_set(got, want, what):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            if not np.array_equal(got[k], want[k]):
                bad = np.flatnonzero(got[k] != want[k])
                raise AssertionError("%s: %s differs at %d places, first %d: %r != %r" % (what, k, len(bad), bad[0], got[k][bad[0]], want[k][bad[0]]))
    assert np.all(got["packed"][-4:] == 0)


def assert_same_layout(lay, host, f, what):
    assert lay.accepted and host.accepted, what
    assert (lay.n_reads, lay.format, lay.max_len, lay.decline_pos) == (host.n_reads, host.format, host.max_len, 0), what
    assert lay.n_reads == f.n_reads and lay.max_len == f.max_len, what
    assert np.array_equal(lay.rec_pos, host.rec_pos) and np.array_equal(lay.seq_off, host.seq_off), what
    assert np.array_equal(lay.seq_off, f.seq_off), what


def check_resident(ca, eng, lay, ref, pad, what):
    f, want, host = ref
    assert_same_layout(lay, host, f, what)
    res = eng.packed()
    assert_same_set(res.arrays(), want[pad], what)
    res.close()
    cnt = eng.counters()
    assert cnt["n_reads"] == want[pad]["n_reads"] and cnt["n_exceptions"] == want[pad]["n_exceptions"], what
    assert cnt["bytes_reads_device"] == 4 * (len(want[pad]["packed"]) - 4), what


def device_copy(data, lead=0):
    """the bytes in a fresh device tensor that starts `lead` bytes behind an aligned allocation"""
    import torch
    big = torch.full((len(data) + lead + 64,), 0x3E, dtype=torch.uint8, device="cuda")      # ('>' around the input: nothing outside it may be read as a record)
    t = big[lead:lead + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    assert t.data_ptr() % 16 == lead % 16
    return big, t


def attach_and_let_go(eng, data, pad, lead=0):
    import torch
    big, t = device_copy(data, lead)
    lay = eng.attach_device_fastx(t, pad_uniform=pad)
    big.fill_(0x40)                                      # the context kept nothing of the bytes: overwrite them, then let them go
    torch.cuda.synchronize()
    del t, big
    torch.cuda.empty_cache()
    return lay


def engine_with_chunk(ca, chunk):
    old = os.environ.pop("CRASS_TEXT_CHUNK_BYTES", None)
    os.environ["CRASS_TEXT_CHUNK_BYTES"] = str(chunk)
    try:
        return ca.SearchEngine()                          # (the switch is read when the context is created)
    finally:
        os.environ.pop("CRASS_TEXT_CHUNK_BYTES", None)
        if old is not None:
            os.environ["CRASS_TEXT_CHUNK_BYTES"] = old


# ---- 1. accepted inputs: the resident set, the layout, the counters ----
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_both_routes_give_the_host_routes_set(ca, eng, tmp_path_factory, name):
    data = INPUTS[name]
    ref = reference(ca, tmp_path_factory, name, data)
    for pad in (0, 1, 2):
        lay = eng.load_fastx_bytes(data, pad_uniform=pad)
        check_resident(ca, eng, lay, ref, pad, "%s pad %d load_fastx_bytes" % (name, pad))
        lay = attach_and_let_go(eng, data, pad)
        check_resident(ca, eng, lay, ref, pad, "%s pad %d attach_device_fastx" % (name, pad))


@pytest.mark.parametrize("name", sorted(EDGE) + ["wrap60", "fq_plain", "fq_odd_quality", "odd_bytes", "one_header"])
def test_device_bytes_at_odd_addresses(ca, eng, tmp_path_factory, name):
    data = INPUTS[name]
    ref = reference(ca, tmp_path_factory, name, data)
    for lead in (1, 3, 7):
        lay = attach_and_let_go(eng, data, 2, lead)
        check_resident(ca, eng, lay, ref, 2, "%s lead %d" % (name, lead))


@pytest.mark.parametrize("chunk", [37, T // 3])
def test_host_bytes_in_small_chunks(ca, tmp_path_factory, chunk):
    with engine_with_chunk(ca, chunk) as e:
        for name in ["wrap60", "fq_crlf", "odd_bytes", "hdr_last_byte_of_tile", "long_seq_line", "fq_four_tiles", "T_plus_1"]:
            ref = reference(ca, tmp_path_factory, name, INPUTS[name])
            lay = e.load_fastx_bytes(INPUTS[name], pad_uniform=2)
            check_resident(ca, e, lay, ref, 2, "%s chunk %d" % (name, chunk))


def test_index_base_and_numpy_input(ca, eng, tmp_path_factory):
    data = INPUTS["uniform150"]
    f, want, host = reference(ca, tmp_path_factory, "uniform150", data)
    lay = eng.load_fastx_bytes(np.frombuffer(data, np.uint8), pad_uniform=2, read_index_base=777)
    assert_same_layout(lay, host, f, "numpy input")
    res = eng.packed()
    got = res.arrays()
    assert got["read_index_base"] == 777 and got["stride_words"] == 10 and got["uniform_len"] == 150 and got["header_id"] is None
    assert np.array_equal(got["packed"], want[2]["packed"])
    res.close()


# ---- 2. declined inputs ----
@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_irregular_inputs_are_declined_and_leave_nothing(ca, eng, tmp_path_factory, name):
    import torch
    data, reason, pos = IRREGULAR[name]
    host = ca.fastx_scan_host(data)
    assert (host.decline_reason, host.decline_pos) == (reason, pos)
    good = INPUTS["one_line"]
    for route in ("host", "device"):
        eng.load_fastx_bytes(good)                        # something resident, so that the decline has something to take away
        with pytest.raises(ca.FastxDeclined) as e:
            if route == "host":
                eng.load_fastx_bytes(data)
            elif len(data):
                attach_and_let_go(eng, data, 2)
            else:
                eng.attach_device_fastx(torch.zeros(0, dtype=torch.uint8, device="cuda"))
        assert e.value.status == 2                       # CRASS_ERR_UNSUPPORTED
        lay = e.value.layout
        assert (lay.decline_reason, lay.decline_pos, lay.n_reads) == (reason, pos, 0), (name, route, lay.decline_reason, lay.decline_pos)
        assert len(lay.rec_pos) == 0 and len(lay.seq_off) == 0
        assert eng.counters()["n_reads"] == 0
        with pytest.raises(ca.CrassError) as e:
            eng.seed_scan()
        assert e.value.status == 6                       # CRASS_ERR_STATE: nothing is resident
    ref = reference(ca, tmp_path_factory, "one_line", good)
    lay = eng.load_fastx_bytes(good, pad_uniform=2)       # ... and the context takes the next regular input
    check_resident(ca, eng, lay, ref, 2, "after " + name)


def test_errors(ca, eng):
    import torch
    lib = ca.load()
    data = np.frombuffer(INPUTS["one_line"], np.uint8)
    dev = torch.from_numpy(data.copy()).to("cuda")
    for fn, ptr in ((lib.crass_hip_load_fastx_bytes, data.ctypes.data), (lib.crass_hip_attach_device_fastx, int(dev.data_ptr()))):
        assert fn(eng.h, None, len(data), 2, 0, None) == 1        # a NULL pointer with n_bytes > 0
        assert fn(eng.h, ptr, len(data), 3, 0, None) == 1         # pad_uniform outside 0 .. 2
        assert fn(None, ptr, len(data), 2, 0, None) == 1
        assert fn(eng.h, None, 0, 2, 0, None) == 2                # an empty file has no format
        assert fn(eng.h, ptr, len(data), 2, 0, None) == 0         # out may be NULL
        assert eng.counters()["n_reads"] == 40
    too_long = b">a\nACGT\n>long\n" + b"ACGT" * 15001 + b"\n>b\nAC\n"      # 60 004 bases
    with pytest.raises(ca.FastxDeclined) as e:
        eng.load_fastx_bytes(too_long)
    assert e.value.status == 2 and (e.value.layout.decline_reason, e.value.layout.decline_pos) == (11, 8)
    assert eng.counters()["n_reads"] == 0
    assert lib.crass_hip_set_header_ids(eng.h, None) == 6         # CRASS_ERR_STATE: no reads
    assert lib.crass_hip_set_header_ids(None, None) == 1
    assert eng.last_scan_ms() == 0.0
    eng.set_stage_timing(1)
    eng.load_fastx_bytes(INPUTS["uniform150"])
    assert eng.last_scan_ms() > 0 and eng.last_pack_ms() > 0
    eng.set_stage_timing(0)


# ---- 3. the same answers through the path ----
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


_synth = {}


def synth_fasta(ca, mates):
    """6 000 synthetic 150-base reads, one in ten with a planted array, as a FASTA wrapped at 60 columns; mates: reads 2 k and
    2 k + 1 share a name"""
    if mates not in _synth:
        n, L = 6000, 150
        words = ca.synth_packed(ca.synth_spec(read_len=L, seed=11, crispr_per_million=100000), 0, n)
        asc = ca.unpack_ascii(words, (L + 15) // 16, L, n)
        seqs = [asc[i * L:(i + 1) * L].tobytes() for i in range(n)]
        data = b"".join(fastx_sets.fa(b"read%d/x comment" % (i // 2 if mates else i), s, 60) for i, s in enumerate(seqs))
        _synth[mates] = (seqs, data)
    return _synth[mates]


def test_same_answers_end_to_end(ca):
    seqs, data = synth_fasta(ca, False)
    buf, off = ca.engine.concat(seqs)
    with ca.SearchEngine() as a, ca.SearchEngine() as b:
        lay = a.load_fastx_bytes(data, pad_uniform=2)
        hid = ca.fastx_header_ids(data, lay.rec_pos)
        assert np.array_equal(hid, np.arange(len(seqs), dtype=np.uint64))
        a.set_header_ids(hid)
        pk = ca.PackedReads((buf, off), pad_uniform=2)
        b.load_reads(pk, header_id=hid)
        ra, rb = run_path(a), run_path(b)
        for x, y, part in zip(ra, rb, ("candidates", "merge", "recruits")):
            assert_same_fields(x, y, part)
        for k in ("n_reads", "n_exceptions", "n_pass1_found", "n_pass2_found", "n_patterns", "bytes_reads_device", "used_fast_filter"):
            assert a.counters()[k] == b.counters()[k], k
        cand, mer, rec = ra
        assert cand.n >= 100 and mer.n_patterns > 0 and rec.n > 0
        found = np.concatenate([cand.read_idx, rec.read_idx])
        text = a.fetch_text(found)
        assert [text[k] for k in range(len(found))] == [seqs[int(r)] for r in found]


def test_set_header_ids_is_loading_with_header_ids(ca):
    seqs, data = synth_fasta(ca, True)
    buf, off = ca.engine.concat(seqs)
    with ca.SearchEngine() as a, ca.SearchEngine() as b:
        lay = a.attach_device_fastx(device_copy(data)[1], pad_uniform=2)
        hid = ca.fastx_header_ids(data, lay.rec_pos)
        assert np.array_equal(hid, (np.arange(len(seqs), dtype=np.uint64) // 2) * 2)
        plain = run_path(a)                               # header ids unset: every read is its own header
        a.set_header_ids(hid)
        cnt = a.counters()
        assert cnt["n_reads"] == len(seqs) and cnt["n_pass1_found"] == 0      # the reads stay, the results are gone
        with pytest.raises(ca.CrassError) as e:
            a.recruits()
        assert e.value.status == 6
        res = a.packed()
        assert np.array_equal(res.arrays()["header_id"], hid)
        res.close()
        pk = ca.PackedReads((buf, off), pad_uniform=2)
        b.load_reads(pk, header_id=hid)
        ra, rb = run_path(a), run_path(b)
        for x, y, part in zip(ra, rb, ("candidates", "merge", "recruits")):
            assert_same_fields(x, y, part)
        assert ra[2].n < plain[2].n                       # mates of pass-1 hits stay out of pass 2
        a.set_header_ids(None)
        again = run_path(a)
        for x, y, part in zip(again, plain, ("candidates", "merge", "recruits")):
            assert_same_fields(x, y, part + " after set_header_ids(None)")
