"""BGZF members inflated on the device (crass_hip_inflate_bgzf_device / crass_hip_load_fastx_bgzf, inflate.hip) against the host
function that runs the same decoder (crass_bgzf_inflate_host, itself held to zlib in tests/test_bgzf_host.py): the text byte for
byte, the verdict field for field on damaged files, guard bytes around the output, and the resident set, layout and counters of
the compressed route against attach_device_fastx on the inflated bytes.  Every comparison is exact equality."""
import gzip
import os

import numpy as np
import pytest

from tests import bgzf_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGULAR = bgzf_sets.regular()
DAMAGED = bgzf_sets.damaged()
NOT_BGZF = bgzf_sets.not_bgzf()
FASTX = bgzf_sets.fastx_regular()
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


@pytest.fixture(scope="module")
def eng_lds(ca):
    """a context whose inflate kernel decodes in the wave's LDS window, not in the output's own range — the other placement — (read when it is created)"""
    os.environ["CRASS_INFLATE_WINDOW"] = "lds"
    try:
        e = ca.SearchEngine()
    finally:
        os.environ.pop("CRASS_INFLATE_WINDOW", None)
    with e:
        yield e


_host = {}


def host_result(ca, key, data):
    """the host function's answer, once per file: (index, text) or (index, verdict)"""
    if key not in _host:
        ix = ca.bgzf_index(data)
        try:
            _host[key] = (ix, ca.bgzf_inflate_host(data, ix))
        except ca.BgzfDeclined as e:
            _host[key] = (ix, e.verdict)
    return _host[key]


def on_device(data, n_text, lead_in=0, lead_out=0):
    """the file in a device tensor that starts lead_in bytes behind an aligned address, and an output tensor lead_out bytes behind
    one, with GUARD marker bytes in front of and behind it"""
    import torch
    big_in = torch.zeros(len(data) + lead_in + 64, dtype=torch.uint8, device="cuda")
    t_in = big_in[lead_in:lead_in + len(data)]
    if len(data):
        t_in.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    big_out = torch.full((GUARD + lead_out + n_text + GUARD,), MARK, dtype=torch.uint8, device="cuda")
    t_out = big_out[GUARD + lead_out:GUARD + lead_out + n_text]
    assert big_in.data_ptr() % 16 == 0 and big_out.data_ptr() % 16 == 0
    return t_in, big_out, t_out


def guards_intact(big_out, lead_out, n_text):
    a = big_out.cpu().numpy()
    return bool(np.all(a[:GUARD + lead_out] == MARK) and np.all(a[GUARD + lead_out + n_text:] == MARK))


def inflate_and_check(ca, eng, key, data, lead_in, lead_out):
    ix, want = host_result(ca, key, data)
    t_in, big_out, t_out = on_device(data, ix.n_text, lead_in, lead_out)
    what = (key, lead_in, lead_out)
    if isinstance(want, tuple):
        with pytest.raises(ca.BgzfDeclined) as e:
            eng.inflate_bgzf_device(t_in, ix, t_out)
        assert e.value.status == 2 and e.value.verdict == want, (what, e.value.verdict, want)
    else:
        assert eng.inflate_bgzf_device(t_in, ix, t_out) == ix.n_text
        got = t_out.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError("%r: the text differs at %d places, first %d" % (what, len(bad), bad[0]))
    assert guards_intact(big_out, lead_out, ix.n_text), what


# ---- 1. the text of every regular file ----
@pytest.mark.parametrize("name", sorted(REGULAR))
def test_device_text_is_the_host_functions(ca, eng, name):
    k = sorted(REGULAR).index(name)
    inflate_and_check(ca, eng, name, REGULAR[name], 0, 0)
    inflate_and_check(ca, eng, name, REGULAR[name], 1 + k % 15, 1 + (7 * k) % 15)


def test_every_lead_of_input_and_output(ca, eng):
    for lead in range(1, 16):
        inflate_and_check(ca, eng, "fastq_edges_on_members", REGULAR["fastq_edges_on_members"], lead, 16 - lead)
        inflate_and_check(ca, eng, "text_65536", REGULAR["text_65536"], 16 - lead, lead)


# ---- 2. damaged files: the host function's verdict, nothing written outside the output ----
@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damaged_files_are_declined_with_the_hosts_verdict(ca, eng, name):
    data, member, reason = DAMAGED[name]
    ix, want = host_result(ca, "damaged " + name, data)
    assert want[:2] == (reason, member)
    inflate_and_check(ca, eng, "damaged " + name, data, 0, 0)
    inflate_and_check(ca, eng, "damaged " + name, data, 5, 11)


def test_single_bit_flips(ca, eng):
    declined = 0
    for i, (data, member) in enumerate(bgzf_sets.bit_flips()):
        key = "flip %d" % i
        inflate_and_check(ca, eng, key, data, i % 16, (3 * i) % 16)
        declined += isinstance(_host[key][1], tuple)
    assert declined >= 150


def test_the_lds_window_placement_gives_the_same(ca, eng_lds):
    """the other placement of the window (CRASS_INFLATE_WINDOW=lds): every regular and damaged file and a quarter of the flips"""
    for k, name in enumerate(sorted(REGULAR)):
        inflate_and_check(ca, eng_lds, name, REGULAR[name], k % 16, (5 * k + 3) % 16)
    for name in sorted(DAMAGED):
        inflate_and_check(ca, eng_lds, "damaged " + name, DAMAGED[name][0], 3, 5)
    for i, (data, member) in enumerate(bgzf_sets.bit_flips()[:50]):
        inflate_and_check(ca, eng_lds, "flip %d" % i, data, i % 16, (3 * i) % 16)
    data = REGULAR["fastq_edges_on_members"]
    want = host_result(ca, "fastq_edges_on_members", data)[1]
    lay = eng_lds.load_fastx_bgzf(data)
    assert lay.n_reads == ca.fastx_scan_host(want).n_reads


def test_errors(ca, eng):
    import torch
    data = REGULAR["members_65"]
    ix, text = host_result(ca, "members_65", data)
    t_in, big_out, t_out = on_device(data, ix.n_text)
    with pytest.raises(ca.CrassError) as e:
        eng.inflate_bgzf_device(t_in, ix, t_out[:ix.n_text - 1])      # out_cap < out_off[n]
    assert e.value.status == 1
    with pytest.raises(ca.CrassError) as e:
        eng.inflate_bgzf_device(t_in[:len(data) - 1], ix, t_out)      # the index reaches beyond n_in
    assert e.value.status == 1
    off = ix.in_off.copy(); off[3], off[4] = off[4], off[3]
    with pytest.raises(ca.CrassError) as e:
        eng.inflate_bgzf_device(t_in, ca.BgzfIndex(off, ix.out_off, ix.data_off), t_out)      # not ascending
    assert e.value.status == 1
    lib = ca.load()
    assert lib.crass_hip_inflate_bgzf_device(eng.h, None, len(data), ix._c(), int(t_out.data_ptr()), ix.n_text, None) == 1
    assert lib.crass_hip_inflate_bgzf_device(None, int(t_in.data_ptr()), len(data), ix._c(), int(t_out.data_ptr()), ix.n_text, None) == 1
    assert guards_intact(big_out, 0, ix.n_text) and bool(torch.all(t_out == MARK))      # nothing was launched
    assert eng.last_inflate_ms() == 0.0
    eng.set_stage_timing(1)
    assert eng.inflate_bgzf_device(t_in, ix, t_out) == ix.n_text
    assert eng.last_inflate_ms() > 0
    eng.set_stage_timing(0)
    assert np.array_equal(t_out.cpu().numpy(), text)


# ---- 3. the compressed route into the resident set ----
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


@pytest.mark.parametrize("name", FASTX)
def test_load_fastx_bgzf_is_attach_on_the_inflated_bytes(ca, eng, name):
    import torch
    data = REGULAR[name]
    ix, text = host_result(ca, name, data)
    dev_text = torch.from_numpy(text.copy()).to("cuda")
    for pad in (0, 1, 2):
        want_lay = eng.attach_device_fastx(dev_text, pad_uniform=pad)
        want = resident(eng)
        lay = eng.load_fastx_bgzf(data, pad_uniform=pad)
        got = resident(eng)
        what = "%s pad %d" % (name, pad)
        assert_same_layout(lay, want_lay, what)
        assert_same_set(got[0], want[0], what)
        assert got[1] == want[1] and got[1]["n_reads"] == lay.n_reads > 0, what


def test_kept_text_serves_header_ids_and_header_lines(ca, eng):
    import torch
    data = REGULAR["fastq_edges_on_members"]
    ix, text = host_result(ca, "fastq_edges_on_members", data)
    big = torch.full((ix.n_text + 100,), MARK, dtype=torch.uint8, device="cuda")
    keep = big[3:]                                       # (an odd address)
    lay = eng.load_fastx_bgzf(data, keep=keep)
    n = int(lay.rec_pos[-1])
    assert n == ix.n_text and np.array_equal(keep[:n].cpu().numpy(), text) and bool(torch.all(keep[n:] == MARK))
    ids, rep = eng.device_header_ids(keep[:n], lay)
    idx = np.array([0, lay.n_reads - 1, 5, 5, 17], dtype=np.uint64)
    lines = eng.fetch_header_lines(keep[:n], lay, idx)
    up = torch.from_numpy(text.copy()).to("cuda")
    ids2, rep2 = eng.device_header_ids(up, lay)
    lines2 = eng.fetch_header_lines(up, lay, idx)
    assert np.array_equal(ids, ids2) and rep == rep2 and np.array_equal(ids, ca.fastx_header_ids(text, lay.rec_pos))
    assert all(np.array_equal(a, b) for a, b in zip(lines, lines2))
    with pytest.raises(ca.CrassError) as e:
        eng.load_fastx_bgzf(data, keep=keep[:n - 1])
    assert e.value.status == 1


def test_declines_leave_nothing_and_the_context_goes_on(ca, eng):
    good = REGULAR["members_1"]
    irregular = b"@a\nACGT\n+\nIIII\n@b\nAC>T\n+\nIIII\n"
    host = ca.fastx_scan_host(irregular)
    assert not host.accepted
    cases = [("scan", bgzf_sets.bgzf(irregular, block=11), None)]
    cases += [("inflate", DAMAGED[k][0], host_result(ca, "damaged " + k, DAMAGED[k][0])[1]) for k in ("crc_byte_flipped", "distance_one_beyond", "deflate_data_cut_short")]
    cases += [("index", NOT_BGZF[k][0], (bgzf_sets.NOT_BGZF, NOT_BGZF[k][1], NOT_BGZF[k][2])) for k in sorted(NOT_BGZF)]
    for kind, data, verdict in cases:
        eng.load_fastx_bgzf(good)                         # something resident, so that the decline has something to take away
        assert eng.counters()["n_reads"] > 0
        if kind == "scan":
            with pytest.raises(ca.FastxDeclined) as e:
                eng.load_fastx_bgzf(data)
            assert (e.value.layout.decline_reason, e.value.layout.decline_pos) == (host.decline_reason, host.decline_pos)
        else:
            with pytest.raises(ca.BgzfDeclined) as e:
                eng.load_fastx_bgzf(data)
            assert e.value.verdict == verdict, (kind, e.value.verdict, verdict)
        assert e.value.status == 2 and eng.counters()["n_reads"] == 0
        with pytest.raises(ca.CrassError) as e:
            eng.seed_scan()
        assert e.value.status == 6                       # CRASS_ERR_STATE: nothing is resident
        eng.load_text([b"ACGTACGTAC", b"GGGTTTAAAC"])
        assert eng.counters()["n_reads"] == 2


# ---- 4. the same answers through the path ----
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


def test_same_records_as_the_uncompressed_route(ca):
    """(tests/golden/data holds no four-line FASTQ the record scan accepts — Ill100.fx is a FASTA it declines —, so the largest
    regular input there stands in: CN_gDC.fa, 4 740 reads)"""
    text = gzip.open(os.path.join(ROOT, "tests", "golden", "data", "CN_gDC.fa.gz"), "rb").read()
    assert ca.fastx_scan_host(text).accepted
    data = bgzf_sets.bgzf(text, block=50021)
    with ca.SearchEngine() as a, ca.SearchEngine() as b:
        la, lb = a.load_fastx_bgzf(data), b.load_fastx_bytes(text)
        assert_same_layout(la, lb, "layout")
        ra, rb = (a.seed_scan(), a.merge(), a.recruit()), (b.seed_scan(), b.merge(), b.recruit())
        for x, y, part in zip(ra, rb, ("candidates", "merge", "recruits")):
            assert_same_fields(x, y, part)
        assert ra[0].n > 0


def test_same_records_from_a_compressed_fastq(ca):
    """the four-line FASTQ route end to end: 3 000 synthetic reads, one in ten with a planted array"""
    n, L = 3000, 150
    words = ca.synth_packed(ca.synth_spec(read_len=L, seed=11, crispr_per_million=100000), 0, n)
    asc = ca.unpack_ascii(words, (L + 15) // 16, L, n)
    text = b"".join(b"@read%d/1 lane=%d\n%s\n+\n%s\n" % (i, i % 4, asc[i * L:(i + 1) * L].tobytes(), b"F:,#F" * (L // 5)) for i in range(n))
    assert ca.fastx_scan_host(text).format == b"@"
    data = bgzf_sets.bgzf(text, block=40009)
    with ca.SearchEngine() as a, ca.SearchEngine() as b:
        la, lb = a.load_fastx_bgzf(data), b.load_fastx_bytes(text)
        assert_same_layout(la, lb, "layout")
        ra, rb = (a.seed_scan(), a.merge(), a.recruit()), (b.seed_scan(), b.merge(), b.recruit())
        for x, y, part in zip(ra, rb, ("candidates", "merge", "recruits")):
            assert_same_fields(x, y, part)
        assert ra[0].n >= 50 and ra[2].n > 0
