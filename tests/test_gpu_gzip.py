"""One plain gzip member inflated on the device chunk by chunk (crass_hip_inflate_gzip_device / crass_hip_load_fastx_gzip /
crass_hip_set_gzip_on_device, gunzip.hip) against the host function that runs the same rule (crass_gzip_inflate_host, itself held
to zlib in tests/test_gzip_host.py): the text byte for byte, the plan (start_bit, link, text_len, n_chain) entry for entry, the
verdict field for field on declined files and bit flips, guard bytes around the output, the overflow protocol, and the resident
set, layout and counters of the compressed routes against the same calls on the text.  Every comparison is exact equality."""
import zlib

import numpy as np
import pytest

from tests import bgzf_sets, gzip_sets

pytestmark = pytest.mark.gpu

REGULAR = gzip_sets.regular()
DECLINED = gzip_sets.declined()
FLIPS = gzip_sets.bit_flips()
GUARD, MARK = 32, 0xA7
ARRAYS = ("packed", "word_off", "lengths", "exc_read", "exc_off", "exc_bytes", "header_id")
SCALARS = ("n_reads", "stride_words", "uniform_len", "n_exceptions", "read_index_base")


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


_host = {}


def plan_tuple(p):
    return (p.n_chunks, p.n_chain, p.start_bit.tolist(), p.link.tolist(), p.text_len.tolist())


def chain_text(plan):
    """the text length the chain of a plan tuple adds up to (what a late decline — CRC, marker — needs as output room)"""
    n_chunks, n_chain, start, link, text_len = plan
    k, total = 0, 0
    for _ in range(n_chain):
        total += text_len[k]
        k = link[k]
        if k >= n_chunks:
            break
    return total


def host_result(ca, key, data, chunk):
    """the host function's answer, once per file and chunk size: (text, plan) or (verdict, plan)"""
    if (key, chunk) not in _host:
        try:
            text, plan = ca.gzip_inflate_host(data, chunk, with_plan=True)
            _host[(key, chunk)] = (text, plan_tuple(plan))
        except ca.BgzfDeclined as e:
            _host[(key, chunk)] = (e.verdict, plan_tuple(e.plan))
    return _host[(key, chunk)]


def on_device(data, n_out, lead_in=0, lead_out=0):
    """the file in a device tensor that starts lead_in bytes behind an aligned address, and an output tensor lead_out bytes behind
    one, with GUARD marker bytes in front of and behind it"""
    import torch
    big_in = torch.zeros(len(data) + lead_in + 64, dtype=torch.uint8, device="cuda")
    t_in = big_in[lead_in:lead_in + len(data)]
    if len(data):
        t_in.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    big_out = torch.full((GUARD + lead_out + n_out + GUARD,), MARK, dtype=torch.uint8, device="cuda")
    t_out = big_out[GUARD + lead_out:GUARD + lead_out + n_out]
    assert big_in.data_ptr() % 16 == 0 and big_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    return t_in, big_out, t_out


def guards_intact(big_out, lead_out, n_out):
    a = big_out.cpu().numpy()
    return bool(np.all(a[:GUARD + lead_out] == MARK) and np.all(a[GUARD + lead_out + n_out:] == MARK))


def inflate_and_check(ca, eng, key, data, chunk, lead_in, lead_out, n_out=None):
    """one device call against the host's answer: returns (device text or verdict, device plan)"""
    want, want_plan = host_result(ca, key, data, chunk)
    what = (key, chunk, lead_in, lead_out)
    declined = isinstance(want, tuple)
    n_out = (chain_text(want_plan) + 64 if declined else len(want)) if n_out is None else n_out
    t_in, big_out, t_out = on_device(data, n_out, lead_in, lead_out)
    if declined:
        with pytest.raises(ca.BgzfDeclined) as e:
            eng.inflate_gzip_device(t_in, t_out, chunk)
        assert e.value.status == 2 and e.value.verdict == want, (what, e.value.verdict, want)
        got_plan = plan_tuple(e.value.plan)
    else:
        n, plan = eng.inflate_gzip_device(t_in, t_out, chunk, with_plan=True)
        assert n == len(want), what
        got = t_out.cpu().numpy()[:n]
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError("%r: the text differs at %d places, first %d" % (what, len(bad), bad[0]))
        got_plan = plan_tuple(plan)
    assert guards_intact(big_out, lead_out, n_out), what
    return got_plan, want_plan


# ---- 1. the text of every regular file at every chunk size ----
@pytest.mark.parametrize("name", sorted(REGULAR))
def test_device_text_is_the_host_functions(ca, eng, name):
    k = sorted(REGULAR).index(name)
    for c, chunk in enumerate(gzip_sets.CHUNKS):
        lead_in, lead_out = (0, 0) if c == 0 else (1 + (k + 5 * c) % 15, 1 + (7 * k + 3 * c) % 15)
        inflate_and_check(ca, eng, name, REGULAR[name][0], chunk, lead_in, lead_out)


def test_every_lead_of_input_and_output(ca, eng):
    for lead in range(1, 16):
        inflate_and_check(ca, eng, "short_blocks", REGULAR["short_blocks"][0], 16384, lead, 16 - lead)
        inflate_and_check(ca, eng, "text_65536", REGULAR["text_65536"][0], 4096, 16 - lead, lead)


# ---- 2. the plan: what k_gz_find found and where k_gz_count linked, entry for entry ----
@pytest.mark.parametrize("name", sorted(REGULAR))
def test_device_plan_is_the_host_functions(ca, eng, name):
    k = sorted(REGULAR).index(name)
    for c, chunk in enumerate(gzip_sets.CHUNKS):
        got, want = inflate_and_check(ca, eng, name, REGULAR[name][0], chunk, (3 * k + c) % 16, (5 * k + 7 * c) % 16)
        assert got[:2] == want[:2], (name, chunk, got[:2], want[:2])
        for part, a, b in zip(("start_bit", "link", "text_len"), got[2:], want[2:]):
            assert a == b, (name, chunk, part, [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:5])


# ---- 3. declined files and bit flips: the host function's verdict; the context goes on ----
def good_file_still_inflates(ca, eng):
    inflate_and_check(ca, eng, "text_32769", REGULAR["text_32769"][0], 4096, 3, 5)


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_files_give_the_hosts_verdict(ca, eng, name):
    data, chunk, reason = DECLINED[name]
    want, _ = host_result(ca, "declined " + name, data, chunk)
    assert isinstance(want, tuple) and want[0] == reason
    got, want_plan = inflate_and_check(ca, eng, "declined " + name, data, chunk, 0, 0)
    assert got == want_plan, name
    got, want_plan = inflate_and_check(ca, eng, "declined " + name, data, chunk, 5, 11)
    assert got == want_plan, name
    good_file_still_inflates(ca, eng)


def test_the_span_inputs_are_accepted_at_a_chunk_where_they_fit(ca, eng):
    for name, (data, chunk, text) in gzip_sets.accepted_at_a_larger_chunk().items():
        assert host_result(ca, "fits " + name, data, chunk)[0].tobytes() == text
        inflate_and_check(ca, eng, "fits " + name, data, chunk, 2, 9)


@pytest.mark.parametrize("part", range(4))
def test_single_bit_flips(ca, eng, part):
    declined = 0
    for i in range(part * 50, part * 50 + 50):
        key = "flip %d" % i
        got, want_plan = inflate_and_check(ca, eng, key, FLIPS[i], gzip_sets.FLIP_CHUNK, i % 16, (3 * i) % 16)
        assert got == want_plan, key
        declined += isinstance(_host[(key, gzip_sets.FLIP_CHUNK)][0], tuple)
    assert declined >= 35
    good_file_still_inflates(ca, eng)


# ---- 4. the overflow protocol and the argument errors ----
def test_overflow_and_errors(ca, eng):
    import torch
    data, text = REGULAR["fasta_level_9"]
    t_in, big_out, t_out = on_device(data, len(text) - 1, 7, 3)
    with pytest.raises(ca.CrassError) as e:
        eng.inflate_gzip_device(t_in, t_out, 16384)           # one byte short
    assert e.value.status == 8 and e.value.n_text == len(text)
    assert bool(torch.all(big_out == MARK))                   # nothing was written
    assert plan_tuple(e.value.plan) == host_result(ca, "fasta_level_9", data, 16384)[1]
    lib = ca.load()
    import ctypes as C
    n = C.c_uint64(0)
    assert lib.crass_hip_inflate_gzip_device(eng.h, None, len(data), 0, int(t_out.data_ptr()), len(text) - 1, C.byref(n), None, None) == 1
    assert lib.crass_hip_inflate_gzip_device(None, int(t_in.data_ptr()), len(data), 0, int(t_out.data_ptr()), len(text) - 1, C.byref(n), None, None) == 1
    assert lib.crass_hip_inflate_gzip_device(eng.h, int(t_in.data_ptr()), len(data), 0, int(t_out.data_ptr()), len(text) - 1, None, None, None) == 1
    assert lib.crass_hip_inflate_gzip_device(eng.h, int(t_in.data_ptr()), len(data), 0, None, 5, C.byref(n), None, None) == 1
    assert bool(torch.all(big_out == MARK))
    # the size query (no output at all), then the stage times
    assert lib.crass_hip_inflate_gzip_device(eng.h, int(t_in.data_ptr()), len(data), 0, None, 0, C.byref(n), None, None) == 8 and n.value == len(text)
    assert eng.last_inflate_ms() == 0.0 and not any(eng.last_gzip_ms().values())
    t_in, big_out, t_out = on_device(data, len(text), 0, 0)
    eng.set_stage_timing(1)
    assert eng.inflate_gzip_device(t_in, t_out, 16384) == len(text)
    ms = eng.last_gzip_ms()
    assert all(ms[k] > 0 for k in ("find", "count", "decode", "windows", "narrow")) and abs(eng.last_inflate_ms() - sum(ms.values())) < 1e-3
    eng.set_stage_timing(0)
    assert t_out.cpu().numpy().tobytes() == text and guards_intact(big_out, 0, len(text))


# ---- 5. the compressed route into the resident set ----
def assert_same_set(got, want, what):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert np.array_equal(got[k], want[k]), (what, k)


def assert_same_layout(a, b, what):
    assert a.accepted and b.accepted, what
    assert (a.n_reads, a.format, a.max_len, a.decline_pos) == (b.n_reads, b.format, b.max_len, b.decline_pos), what
    assert np.array_equal(a.rec_pos, b.rec_pos) and np.array_equal(a.seq_off, b.seq_off), what


def resident(eng):
    res = eng.packed()
    arrays = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in res.arrays().items()}
    res.close()
    cnt = eng.counters()
    return arrays, {k: cnt[k] for k in ("n_reads", "n_exceptions", "bytes_reads_device")}


@pytest.mark.parametrize("name,pads", [("fastq_level_6", (0, 1, 2)), ("fasta_level_6", (2,))])
def test_load_fastx_gzip_is_attach_on_the_inflated_bytes(ca, eng, name, pads):
    import torch
    assert name in gzip_sets.fastx_regular()
    data, _ = REGULAR[name]
    text = zlib.decompress(data, 31)
    dev_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to("cuda")
    for pad in pads:
        want_lay = eng.attach_device_fastx(dev_text, pad_uniform=pad)
        want = resident(eng)
        lay = eng.load_fastx_gzip(data, pad_uniform=pad)
        got = resident(eng)
        what = "%s pad %d" % (name, pad)
        assert_same_layout(lay, want_lay, what)
        assert_same_set(got[0], want[0], what)
        assert got[1] == want[1] and got[1]["n_reads"] == lay.n_reads > 0, what
        if name.startswith("fasta"):
            assert got[1]["n_exceptions"] > 0                # (reads with N)
        assert len(set(np.diff(lay.seq_off).tolist())) > 10   # (ragged lengths)


def test_kept_text_serves_header_ids_and_header_lines(ca, eng):
    import torch
    data, text = REGULAR["fastq_level_1"]              # (whole records; three chunks at the default chunk size)
    want = np.frombuffer(text, np.uint8)
    big = torch.full((len(text) + 100,), MARK, dtype=torch.uint8, device="cuda")
    keep = big[3:]                                       # (an odd address)
    lay = eng.load_fastx_gzip(data, keep=keep)
    n = int(lay.rec_pos[-1])
    assert n == len(text) and np.array_equal(keep[:n].cpu().numpy(), want) and bool(torch.all(keep[n:] == MARK)) and bool(torch.all(big[:3] == MARK))
    ids, rep = eng.device_header_ids(keep[:n], lay)
    idx = np.array([0, lay.n_reads - 1, 5, 5, 17], dtype=np.uint64)
    lines = eng.fetch_header_lines(keep[:n], lay, idx)
    up = torch.from_numpy(want.copy()).to("cuda")
    ids2, rep2 = eng.device_header_ids(up, lay)
    lines2 = eng.fetch_header_lines(up, lay, idx)
    assert np.array_equal(ids, ids2) and rep == rep2 and np.array_equal(ids, ca.fastx_header_ids(want, lay.rec_pos))
    assert all(np.array_equal(a, b) for a, b in zip(lines, lines2))
    with pytest.raises(ca.CrassError) as e:
        eng.load_fastx_gzip(data, keep=keep[:n - 1])
    assert e.value.status == 1
    with pytest.raises(ca.CrassError) as e:
        eng.seed_scan()
    assert e.value.status == 6                           # CRASS_ERR_STATE: nothing is resident


def test_declines_leave_nothing_and_the_context_goes_on(ca, eng):
    good = gzip_sets.gz(gzip_sets.fastq(81, 100000))
    irregular = b"@a\nACGT\n+\nIIII\n@b\nAC>T\n+\nIIII\n"
    host = ca.fastx_scan_host(irregular)
    assert not host.accepted
    cases = [("scan", gzip_sets.gz(irregular), None)]
    for k in ("crc_byte_flipped", "two_members", "cut_before_the_flags", "block_type_3"):
        cases.append(("inflate", DECLINED[k][0], host_result(ca, "declined0 " + k, DECLINED[k][0], 0)[0]))
    cases.append(("inflate", bgzf_sets.bgzf(b">a\nACGT\n"), host_result(ca, "a bgzf file", bgzf_sets.bgzf(b">a\nACGT\n"), 0)[0]))      # (several members: reason 13)
    for kind, data, verdict in cases:
        eng.load_fastx_gzip(good)                         # something resident, so that the decline has something to take away
        assert eng.counters()["n_reads"] > 0
        if kind == "scan":
            with pytest.raises(ca.FastxDeclined) as e:
                eng.load_fastx_gzip(data)
            assert (e.value.layout.decline_reason, e.value.layout.decline_pos) == (host.decline_reason, host.decline_pos)
        else:
            assert isinstance(verdict, tuple)
            with pytest.raises(ca.BgzfDeclined) as e:
                eng.load_fastx_gzip(data)
            assert e.value.verdict == verdict, (kind, e.value.verdict, verdict)
        assert e.value.status == 2 and eng.counters()["n_reads"] == 0
        eng.load_text([b"ACGTACGTAC", b"GGGTTTAAAC"])
        assert eng.counters()["n_reads"] == 2


# ---- 6. the files route ----
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


def test_files_route_with_the_switch_on_and_off(ca):
    plain = gzip_sets.fastq(71, 60000)
    text = gzip_sets.fasta(72, 700000)
    zipped = gzip_sets.gz(text, level=6)
    assert len(zipped) > 2 * 65536
    blocked = bgzf_sets.bgzf(gzip_sets.fastq(73, 150000), block=30011)
    with ca.SearchEngine() as e:
        # off (the default): the decline of today
        with pytest.raises(ca.FastxFilesDeclined) as d:
            e.load_fastx_files([plain, zipped, blocked])
        assert d.value.status == 2 and d.value.layout.verdict == (1, 0, 0, (bgzf_sets.NOT_BGZF, 0, 0))
        want_lay = e.load_fastx_files([plain, text, blocked])
        want = resident(e)
        want_arena = e.resident_fastx()[1]
        e.set_gzip_on_device(True)
        lay = e.load_fastx_files([plain, zipped, blocked])
        got = resident(e)
        assert_same_fields(lay, want_lay, "files layout")
        assert_same_set(got[0], want[0], "files")
        assert got[1] == want[1] and e.resident_fastx()[1] == want_arena
        assert int(lay.file_byte_base[2]) - int(lay.file_byte_base[1]) == len(text) + 1      # (the count step sized the gzip file's share of the arena)
        # a damaged gzip file declines the set with the host function's verdict for that file
        bad = bytearray(zipped); bad[-7] ^= 0x40
        with pytest.raises(ca.FastxFilesDeclined) as d:
            e.load_fastx_files([plain, bytes(bad), blocked])
        assert d.value.layout.verdict == (1, 0, 0, (gzip_sets.CRC, 0, 0))
        # ... and off again
        e.set_gzip_on_device(False)
        with pytest.raises(ca.FastxFilesDeclined) as d:
            e.load_fastx_files([plain, zipped, blocked])
        assert d.value.layout.verdict == (1, 0, 0, (bgzf_sets.NOT_BGZF, 0, 0))
