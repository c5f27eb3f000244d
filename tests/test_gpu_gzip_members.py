"""Plain gzip of several members inflated on the device (crass_hip_inflate_gzip_members_device / crass_hip_load_fastx_gzip_members /
crass_hip_set_gzip_on_device(2), gunzip.hip) against the host function that runs the same rule (crass_gzip_inflate_members_host,
itself held to the strict zlib loop in tests/test_gzip_members_host.py): the text byte for byte, plan and members entry for entry,
the verdict field for field on declined files and bit flips, guard bytes around the output, the overflow protocol, and the
resident set, layout and counters of the compressed routes against the same calls on the text.  Every comparison is exact equality."""
import numpy as np
import pytest

from tests import bgzf_sets
from tests import gzip_member_sets as sets

pytestmark = pytest.mark.gpu

REGULAR = sets.regular()
DECLINED, OFFS = sets.declined()
FLIPS = sets.bit_flips()
GUARD, MARK = 32, 0xA7
LEADS = ((0, 0), (1, 15), (7, 1), (15, 7))
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


def members_tuple(m):
    return (m.n_members, m.in_off.tolist(), m.text_off.tolist())


def chain_text(plan):
    n_chunks, n_chain, start, link, text_len = plan
    k, total = 0, 0
    for _ in range(n_chain):
        total += text_len[k]
        k = link[k]
        if k >= n_chunks:
            break
    return total


def host_result(ca, key, data, chunk):
    """the host function's answer, once per file and chunk size: (text, plan, members) or (verdict, plan, None)"""
    if (key, chunk) not in _host:
        try:
            text, plan, members = ca.gzip_inflate_members_host(data, chunk, with_plan=True)
            _host[(key, chunk)] = (text, plan_tuple(plan), members_tuple(members))
        except ca.BgzfDeclined as e:
            _host[(key, chunk)] = (e.verdict, plan_tuple(e.plan), None)
    return _host[(key, chunk)]


def on_device(data, n_out, lead_in=0, lead_out=0):
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


def inflate_and_check(ca, eng, key, data, chunk, lead_in, lead_out):
    """one device call against the host's answer in every field"""
    want, want_plan, want_members = host_result(ca, key, data, chunk)
    what = (key, chunk, lead_in, lead_out)
    declined = isinstance(want, tuple)
    n_out = chain_text(want_plan) + 64 if declined else len(want)
    t_in, big_out, t_out = on_device(data, n_out, lead_in, lead_out)
    if declined:
        with pytest.raises(ca.BgzfDeclined) as e:
            eng.inflate_gzip_members_device(t_in, t_out, chunk)
        assert e.value.status == 2 and e.value.verdict == want, (what, e.value.verdict, want)
        got_plan = plan_tuple(e.value.plan)
    else:
        n, plan, members = eng.inflate_gzip_members_device(t_in, t_out, chunk, with_plan=True)
        assert n == len(want), what
        got = t_out.cpu().numpy()[:n]
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError("%r: the text differs at %d places, first %d" % (what, len(bad), bad[0]))
        got_plan = plan_tuple(plan)
        assert members_tuple(members) == want_members, what
    assert guards_intact(big_out, lead_out, n_out), what
    assert got_plan[:2] == want_plan[:2], (what, got_plan[:2], want_plan[:2])
    for part, a, b in zip(("start_bit", "link", "text_len"), got_plan[2:], want_plan[2:]):
        assert a == b, (what, part, [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:5])
    return want


# ---- 1. text, plan and members of every regular file at every chunk size, at input / output leads 0, 1, 7, 15 ----
@pytest.mark.parametrize("name", sorted(REGULAR))
def test_device_answer_is_the_host_functions(ca, eng, name):
    k = sorted(REGULAR).index(name)
    for c, chunk in enumerate(sets.CHUNKS):
        lead_in, lead_out = LEADS[(c + k) % 4]
        want = inflate_and_check(ca, eng, name, REGULAR[name], chunk, lead_in, lead_out)
        assert not isinstance(want, tuple), (name, chunk, want)


def test_every_lead_pair_on_a_small_file(ca, eng):
    for lead_in in (0, 1, 7, 15):
        for lead_out in (0, 1, 7, 15):
            inflate_and_check(ca, eng, "bgzf_as_plain", REGULAR["bgzf_as_plain"], 4096, lead_in, lead_out)


# ---- 2. declined files and bit flips: the host function's verdict; the context goes on ----
def good_file_still_inflates(ca, eng):
    inflate_and_check(ca, eng, "bgzf_as_plain", REGULAR["bgzf_as_plain"], 4096, 3, 5)


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_files_give_the_hosts_verdict(ca, eng, name):
    data, chunk, reason, member = DECLINED[name]
    want = host_result(ca, "declined " + name, data, chunk)[0]
    assert isinstance(want, tuple) and want[0] == reason
    if member is not None:
        assert want == (reason, member, OFFS[member])
    inflate_and_check(ca, eng, "declined " + name, data, chunk, 0, 0)
    inflate_and_check(ca, eng, "declined " + name, data, chunk, 7, 15)
    for other in sets.CHUNKS:
        if other != chunk and not name.startswith("distance"):
            inflate_and_check(ca, eng, "declined " + name, data, other, 1, 1)
    good_file_still_inflates(ca, eng)


@pytest.mark.parametrize("part", range(4))
def test_single_bit_flips(ca, eng, part):
    declined = 0
    for i in range(part * 100, part * 100 + 100):
        key = "flip %d" % i
        want = inflate_and_check(ca, eng, key, FLIPS[i], sets.FLIP_CHUNK, i % 16, (3 * i) % 16)
        declined += isinstance(want, tuple)
    assert declined >= 75
    good_file_still_inflates(ca, eng)


# ---- 3. the overflow protocol and the argument errors ----
def test_overflow_and_errors(ca, eng):
    import ctypes as C
    import torch
    data = REGULAR["inner_headers_all_four"]
    text, want_plan, want_members = host_result(ca, "inner_headers_all_four", data, 16384)
    t_in, big_out, t_out = on_device(data, len(text) - 1, 7, 1)
    with pytest.raises(ca.CrassError) as e:
        eng.inflate_gzip_members_device(t_in, t_out, 16384)       # one byte short
    assert e.value.status == 8 and e.value.n_text == len(text)
    assert bool(torch.all(big_out == MARK))                       # nothing was stored
    assert plan_tuple(e.value.plan) == want_plan
    lib = ca.load()
    fn = lib.crass_hip_inflate_gzip_members_device
    n, mc = C.c_uint64(0), ca._abi.GzipMembersC()
    assert fn(eng.h, None, len(data), 0, int(t_out.data_ptr()), len(text) - 1, C.byref(n), None, None, None) == 1
    assert fn(None, int(t_in.data_ptr()), len(data), 0, int(t_out.data_ptr()), len(text) - 1, C.byref(n), None, None, None) == 1
    assert fn(eng.h, int(t_in.data_ptr()), len(data), 0, int(t_out.data_ptr()), len(text) - 1, None, None, None, None) == 1
    assert fn(eng.h, int(t_in.data_ptr()), len(data), 0, None, 5, C.byref(n), None, None, None) == 1
    assert fn(eng.h, int(t_in.data_ptr()), len(data), 0, None, 0, C.byref(n), None, C.byref(mc), None) == 8 and n.value == len(text)
    assert mc.n_members == 0 and not mc.in_off                    # (the table comes with the text)
    assert bool(torch.all(big_out == MARK))
    t_in, big_out, t_out = on_device(data, len(text), 0, 0)
    eng.set_stage_timing(1)
    assert eng.inflate_gzip_members_device(t_in, t_out, 16384) == len(text)
    ms = eng.last_gzip_ms()
    assert all(ms[k] > 0 for k in ("find", "count", "decode", "windows", "narrow")) and abs(eng.last_inflate_ms() - sum(ms.values())) < 1e-3
    eng.set_stage_timing(0)
    assert np.array_equal(t_out.cpu().numpy(), text) and guards_intact(big_out, 0, len(text))
    # the single-member device call goes on declining the file
    with pytest.raises(ca.BgzfDeclined) as e:
        eng.inflate_gzip_device(t_in, t_out, 16384)
    assert e.value.reason == sets.TRAILING


# ---- 4. the compressed route into the resident set ----
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


@pytest.mark.parametrize("name", ["record_boundary", "inside_a_quality_line"])
def test_load_fastx_gzip_members_is_attach_on_the_inflated_bytes(ca, eng, name):
    import torch
    data, text = sets.fastx_members()[name]
    _, in_off, text_off = sets.strict(data)
    dev_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to("cuda")
    for pad in (0, 2):
        want_lay = eng.attach_device_fastx(dev_text, pad_uniform=pad)
        want = resident(eng)
        lay, members = eng.load_fastx_gzip_members(data, pad_uniform=pad, with_members=True)
        got = resident(eng)
        what = "%s pad %d" % (name, pad)
        assert_same_layout(lay, want_lay, what)
        assert_same_set(got[0], want[0], what)
        assert got[1] == want[1] and got[1]["n_reads"] == lay.n_reads > 0, what
        assert members_tuple(members) == (len(in_off) - 1, in_off, text_off), what
    # the single-member route goes on declining it, and leaves nothing
    with pytest.raises(ca.BgzfDeclined) as e:
        eng.load_fastx_gzip(data)
    assert e.value.reason == sets.TRAILING and eng.counters()["n_reads"] == 0
    # a damaged member declines the members route with the host function's verdict
    bad = bytearray(data); bad[in_off[1] - 7] ^= 0x40
    eng.load_fastx_gzip_members(data)
    with pytest.raises(ca.BgzfDeclined) as e:
        eng.load_fastx_gzip_members(bytes(bad))
    assert e.value.verdict == (sets.CRC, 0, 0) and eng.counters()["n_reads"] == 0


# ---- 5. the files route ----
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


def test_files_route_with_the_switch_at_2_1_and_0(ca):
    plain = sets.fastq(171, 60000)
    zipped, text = sets.fastx_members()["inside_a_quality_line"]
    single = sets.gz(sets.fasta(172, 300000))
    single_text = sets.strict(single)[0]
    blocked = bgzf_sets.bgzf(sets.fastq(173, 150000), block=30011)
    with ca.SearchEngine() as e:
        want_lay = e.load_fastx_files([plain, text, single_text, blocked])
        want = resident(e)
        want_arena = e.resident_fastx()[1]
        # 0 (the default) and 1: the declines of today
        with pytest.raises(ca.FastxFilesDeclined) as d:
            e.load_fastx_files([plain, zipped, single, blocked])
        assert d.value.status == 2 and d.value.layout.verdict == (1, 0, 0, (bgzf_sets.NOT_BGZF, 0, 0))
        e.set_gzip_on_device(True)
        with pytest.raises(ca.FastxFilesDeclined) as d:
            e.load_fastx_files([plain, zipped, single, blocked])
        try:
            ca.gzip_inflate_host(zipped, 0)
            raise AssertionError("the single-member rule took a file of two members")
        except ca.BgzfDeclined as one:
            assert one.reason == sets.TRAILING
            assert d.value.layout.verdict == (1, 0, 0, one.verdict)
        # 2: the same set as from the plain text
        e.set_gzip_on_device(True, members=True)
        lay = e.load_fastx_files([plain, zipped, single, blocked])
        got = resident(e)
        assert_same_fields(lay, want_lay, "files layout")
        assert_same_set(got[0], want[0], "files")
        assert got[1] == want[1] and e.resident_fastx()[1] == want_arena
        assert int(lay.file_byte_base[2]) - int(lay.file_byte_base[1]) == len(text) + 1      # (the count step sized the file's share of the arena)
        # a damaged member declines the set with the host function's verdict for that file
        at = sets.strict(zipped)[1][1]
        bad = bytearray(zipped); bad[-7] ^= 0x40
        with pytest.raises(ca.FastxFilesDeclined) as d:
            e.load_fastx_files([plain, bytes(bad), single, blocked])
        assert d.value.layout.verdict == (1, 0, 0, (sets.CRC, 1, at))
        # ... and off again
        e.set_gzip_on_device(False)
        with pytest.raises(ca.FastxFilesDeclined) as d:
            e.load_fastx_files([plain, zipped, single, blocked])
        assert d.value.layout.verdict == (1, 0, 0, (bgzf_sets.NOT_BGZF, 0, 0))
