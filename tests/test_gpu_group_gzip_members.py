"""Plain gzip of several members across the ranks of a group (crass_hip_group_inflate_gzip_members: k_gz_find_members /
k_gz_count_members over each rank's chunks, k_gz_decode_members / k_gz_windows_sym_members over its elements, the member table and
the CRC pieces made on the host, k_gz_window_resolve / k_gz_narrow_members / k_gz_member_crc), and the files load that takes such
files (crass_hip_group_set_gzip_on_device with mode 2), against the host statements (crass_gzip_inflate_members_ranges_host,
crass_fastx_files_shards_host_gzip with gzip_mode 2), the same load on the inflated files and the single context's members load.
Groups of 2, 3 and 4 contexts share device 0 (local copies), one group per size; chunk 4096 throughout.  Every comparison is
exact equality."""
import zlib

import numpy as np
import pytest

from tests import bgzf_sets, group_gzip_member_sets as gms, gzip_member_sets as sets, gzip_sets
from tests.test_gpu_group_gzip import wrapped_fastq

pytestmark = pytest.mark.gpu

REGULAR = sets.regular()
FASTX = sets.fastx_members()
DECLINED, OFFS = sets.declined()
DESIGNED = gms.designed()
CHUNK = gms.CHUNK
SIZES = (2, 3, 4)


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def groups(ca):
    """one group per number of ranks, made on first use, with the switch at 2 (chunk 4096)"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = ca.SearchGroup([0] * n, local_copies=True)
            made[n].set_gzip_on_device(2, CHUNK)
        return made[n]
    yield get
    for g in made.values():
        g.close()


@pytest.fixture(scope="module")
def eng(ca):
    with ca.SearchEngine() as e:
        e.set_gzip_on_device(True, members=True)
        yield e


def plan_tuple(p):
    return (p.n_chunks, p.n_chain, p.start_bit.tolist(), p.link.tolist(), p.text_len.tolist())


def members_tuple(m):
    return (m.n_members, m.in_off.tolist(), m.text_off.tolist())


_host = {}


def host_ranges(ca, key, data, n, nominal=None, chunk=CHUNK):
    """crass_gzip_inflate_members_ranges_host's answer, once per file, number of ranges and cuts: (text, plan, members) or
    (verdict, plan)"""
    k = (key, n, chunk, None if nominal is None else tuple(nominal))
    if k not in _host:
        try:
            text, plan, members = ca.gzip_inflate_members_ranges_host(data, n, chunk, nominal=nominal, with_plan=True)
            _host[k] = (text, plan_tuple(plan), members_tuple(members))
        except ca.BgzfDeclined as e:
            _host[k] = (e.verdict, plan_tuple(e.plan))
    return _host[k]


def inflate_and_check(ca, g, key, data, nominal=None, chunk=CHUNK):
    want = host_ranges(ca, key, data, g.n, nominal, chunk)
    what = (key, g.n, nominal)
    if len(want) == 2:
        with pytest.raises(ca.BgzfDeclined) as e:
            g.inflate_gzip_members(data, chunk, nominal=nominal)
        assert e.value.status == 2 and e.value.verdict == want[0], (what, e.value.verdict, want[0])
        assert plan_tuple(e.value.plan) == want[1], what
        return None
    got, plan, members = g.inflate_gzip_members(data, chunk, nominal=nominal, with_plan=True)
    assert len(got) == len(want[0]), what
    if not np.array_equal(got, want[0]):
        bad = np.flatnonzero(got != want[0])
        raise AssertionError("%r: the text differs at %d places, first %d" % (what, len(bad), bad[0]))
    assert plan_tuple(plan) == want[1] and members_tuple(members) == want[2], what
    return plan, members


# ---- 1. the distributed inflate ----
@pytest.mark.parametrize("n", SIZES)
def test_text_plan_members_and_verdict_are_the_host_functions(ca, groups, n):
    g = groups(n)
    for name in sorted(REGULAR):
        plan, members = inflate_and_check(ca, g, name, REGULAR[name])
        c = g.gzip_members_counters()
        assert c[0] == 1 and c[1] == members.n_members and c[2] >= int(np.count_nonzero(np.diff(members.text_off))), (name, c)
    plan, members = inflate_and_check(ca, g, "designed", DESIGNED[0])
    assert g.gzip_members_counters()[1] == 8
    for name in sorted(DECLINED):
        data, chunk, reason, member = DECLINED[name]
        inflate_and_check(ca, g, "declined " + name, data, chunk=chunk)
        assert host_ranges(ca, "declined " + name, data, n, chunk=chunk)[0][0] == reason
    inflate_and_check(ca, g, "designed", DESIGNED[0])      # (the group goes on behind a decline)


@pytest.mark.parametrize("n", SIZES)
def test_designed_cuts_on_the_designed_file(ca, groups, n):
    g = groups(n)
    data, text = DESIGNED
    _, plan, members = ca.gzip_inflate_members_host(data, CHUNK, with_plan=True)
    off = gms.check_designed(data, text, plan, members)
    cuts = {k: v for k, v in gms.designed_cuts(off).items() if len(v) == n - 1}
    assert len(cuts) >= 15
    for what, nominal in sorted(cuts.items()):
        inflate_and_check(ca, g, "designed", data, nominal)
        c = g.gzip_members_counters()
        assert c[:2] == (1, 8), (what, c)


def first_elements(off, cuts):
    """the rule of gz_elements_for, restated: the first element of every range [cuts[r], cuts[r + 1])"""
    ends = np.asarray(off[1:], dtype=np.int64)
    return [0 if a == 0 else int(np.searchsorted(ends, a, side="right")) for a in cuts[:-1]]


@pytest.mark.parametrize("n", SIZES)
def test_a_range_that_holds_a_boundary_exports_no_reference(ca, groups, n):
    """many_single_block_members: every chain element begins a member or holds a boundary, so with even cuts every window a rank
    exports is free of references — from the dead-entry rule, whatever the text"""
    g = groups(n)
    data = REGULAR["many_single_block_members"]
    plan, members = inflate_and_check(ca, g, "many_single_block_members", data)
    off = gms.ggs.chain_offsets(plan)
    T = off[-1]
    e0 = first_elements(off, [T // n * r + T % n * r // n for r in range(n)] + [T])
    exporting = sum(1 for r in range(n - 1) if e0[r] < e0[r + 1] < plan.n_chain)
    c = g.gzip_members_counters()
    assert exporting == n - 1 and c == (1, 120, c[2], exporting), (c, exporting)


def flips_by_kind(ca):
    """the first flip of every outcome kind among bit_flips(): the chain declines it, a member's ISIZE, a member's CRC-32, and a
    marker where there is one"""
    out = {}
    for i, data in enumerate(sets.bit_flips()):
        try:
            ca.gzip_inflate_members_host(data, sets.FLIP_CHUNK)
        except ca.BgzfDeclined as e:
            kind = ("crc" if e.reason == sets.CRC else "marker" if e.reason == sets.MARKER else "isize" if e.reason in (sets.OUTPUT_LONG, sets.OUTPUT_SHORT)
                    else "chain")
            out.setdefault(kind, (i, data))
    return out


def test_flips_of_every_outcome_kind(ca, groups):
    flips = flips_by_kind(ca)
    assert {"chain", "isize", "crc"} <= set(flips), sorted(flips)
    for n in (2, 3):
        g = groups(n)
        for kind, (i, data) in sorted(flips.items()):
            inflate_and_check(ca, g, "flip %d" % i, data, chunk=sets.FLIP_CHUNK)


def test_overflow_protocol_and_argument_errors(ca, groups):
    import ctypes as C
    g = groups(3)
    data = REGULAR["empty_members_everywhere"]
    text = sets.strict(data)[0]
    with pytest.raises(ca.CrassError) as e:
        g.inflate_gzip_members(data, CHUNK, out_cap=len(text) - 1)
    assert e.value.status == 8 and e.value.n_text == len(text) and not e.value.out.any()
    a = np.frombuffer(data, np.uint8)
    n = C.c_uint64(0)
    out = np.zeros(len(text), np.uint8)
    f = g.lib.crass_hip_group_inflate_gzip_members
    assert f(g.h, a.ctypes.data, len(a), CHUNK, None, None, 0, C.byref(n), None, None, None) == 8 and n.value == len(text)
    assert f(None, a.ctypes.data, len(a), CHUNK, None, out.ctypes.data, len(out), C.byref(n), None, None, None) == 1
    assert f(g.h, a.ctypes.data, len(a), CHUNK, None, out.ctypes.data, len(out), None, None, None, None) == 1
    nom = np.asarray([5, 4], np.uint64)
    assert f(g.h, a.ctypes.data, len(a), CHUNK, nom.ctypes.data, out.ctypes.data, len(out), C.byref(n), None, None, None) == 1
    assert f(g.h, a.ctypes.data, len(a), CHUNK, None, out.ctypes.data, len(out), C.byref(n), None, None, None) == 0 and out.tobytes() == text
    # the single-member seam goes on declining the file
    with pytest.raises(ca.BgzfDeclined) as d:
        g.inflate_gzip(data, CHUNK)
    assert d.value.reason == sets.TRAILING and g.gzip_members_counters() == (0, 0, 0, 0)
    # the member CRC pass has a time of its own, beside narrow's
    assert not any(g.gzip_members_ms(r)["member_crc"] for r in range(3))
    for r in range(3):
        g.rank_set_stage_timing(r, 1)
    assert g.inflate_gzip_members(data, CHUNK).tobytes() == text
    for r in range(3):
        ms = g.gzip_ms(r)
        assert all(ms[k] > 0 for k in ("find", "count", "decode", "windows_sym", "narrow")) and g.gzip_members_ms(r)["member_crc"] > 0, (r, ms)
        g.rank_set_stage_timing(r, 0)


# ---- 2. the files load with the switch at 2 ----
def records_of_group(g, n):
    idx = np.arange(n, dtype=np.uint64)
    t = g.fetch_text(idx)
    return {"n": n, "text": (t.chars[:int(t.off[-1])].copy(), t.off.copy()), "lines": g.fetch_header_lines(idx), "quality": g.fetch_quality(idx),
            "comments": g.fetch_comments(idx)}


def records_of_engine(eng, files):
    lay = eng.load_fastx_files(files)
    idx = np.arange(lay.n_reads, dtype=np.uint64)
    t = eng.fetch_text(idx)
    addr, nb = eng.resident_fastx()
    return {"n": lay.n_reads, "text": (t.chars[:int(t.off[-1])].copy(), t.off.copy()), "lines": eng.fetch_header_lines(addr, np.append(lay.rec_pos[:-1], nb), idx),
            "quality": eng.fetch_quality(addr, nb, lay.rec_pos, idx), "comments": eng.fetch_comments(idx)}


def assert_same_records(got, want, what):
    assert got["n"] == want["n"] > 0, what
    assert np.array_equal(got["text"][1], want["text"][1]) and np.array_equal(got["text"][0], want["text"][0]), (what, "text")
    for k in ("lines", "quality", "comments"):
        a, b = got[k], want[k]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0][:int(a[1][-1])], b[0][:int(b[1][-1])]) and np.array_equal(a[2], b[2]), (what, k)


def same_shards(a, b, what):
    assert a.verdict == b.verdict and (a.n_ranks, a.n_files, a.n_reads, a.max_len) == (b.n_ranks, b.n_files, b.n_reads, b.max_len), what
    for k in ("rank_read_base", "cut_file", "cut_pos", "file_read_base"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)
    assert a.formats == b.formats, what


def jobs():
    """name -> (files as given, the same with every plain gzip file inflated, members of the gzip files summed)"""
    out = {k: ([data], [text], len(sets.strict(data)[1]) - 1) for k, (data, text) in FASTX.items()}
    out["designed"] = ([DESIGNED[0]], [DESIGNED[1]], 8)
    r1, r2, fq2 = gzip_sets.fastq(104, 200000), gzip_sets.fastq(105, 200000), gzip_sets.fastq(103, 120000)
    cut = [0, 50001, 120000, len(r1)]
    many = b"".join(gzip_sets.gz(r1[a:b], level=lv, flushes=[(p, zlib.Z_BLOCK) for p in range(7000, b - a, 7000)]) for a, b, lv in zip(cut, cut[1:], (1, 6, 9)))
    blocked = bgzf_sets.bgzf(fq2, block=30011)
    out["paired"] = ([many, gzip_sets.gz(r2, level=9), blocked], [r1, r2, blocked], 4)
    return out


JOBS = jobs()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("job", sorted(JOBS))
def test_load_with_members_files_is_the_load_of_their_text(ca, groups, eng, job, n):
    g = groups(n)
    zipped, plain, n_members = JOBS[job]
    sh = g.load_fastx_files(zipped)
    same_shards(sh, ca.fastx_files_shards_host_gzip(zipped, n, gzip_mode=2, chunk_bytes=CHUNK), (job, n))
    n_gz = sum(1 for z, p in zip(zipped, plain) if z is not p)
    c, cm = g.gzip_counters(), g.gzip_members_counters()
    assert c[0] == n_gz and cm[0] == n_gz and cm[1] == n_members and cm[2] >= n_members - 1, (c, cm)
    got = records_of_group(g, sh.n_reads)
    g.load_fastx_files(plain)
    assert g.gzip_counters() == (0,) * 6 and g.gzip_members_counters() == (0,) * 4
    assert_same_records(got, records_of_group(g, sh.n_reads), (job, n, "the same load on the text"))
    assert_same_records(got, records_of_engine(eng, zipped), (job, n, "one context, members on device"))
    g.load_fastx_files(zipped)
    g.step()                                              # (the search path runs on what was loaded)


def test_mode_1_is_unchanged_and_mode_2_then_takes_the_file(ca, groups):
    g = groups(2)
    zipped, plain, _ = JOBS["paired"]
    try:
        g.set_gzip_on_device(1, CHUNK)
        with pytest.raises(ca.FastxFilesDeclined) as d:
            g.load_fastx_files(zipped)
        want = ca.fastx_files_shards_host_gzip(zipped, 2, gzip_mode=1, chunk_bytes=CHUNK)
        assert d.value.status == 2 and d.value.layout.verdict == want.verdict and want.verdict[0] == 0 and want.verdict[3][0] == sets.TRAILING == 13
        assert g.gzip_members_counters() == (0,) * 4
        # a single-member file: mode 2 gives what mode 1 gives
        one = [gzip_sets.gz(plain[1], level=9)]
        a = g.load_fastx_files(one)
        ra = records_of_group(g, a.n_reads)
    finally:
        g.set_gzip_on_device(2, CHUNK)
    b = g.load_fastx_files(one)
    same_shards(a, b, "one member")
    assert_same_records(ra, records_of_group(g, b.n_reads), "one member")
    assert g.gzip_members_counters()[:2] == (1, 1)
    assert g.load_fastx_files(zipped).accepted


def test_wrapped_fastq_in_three_members(ca, monkeypatch):
    """records of 16 to 40 KB over three members with short blocks (the boundaries inside records): a margin of 64 bytes that
    doubles until a record ends has the ranks pull further elements through the seeded walk, in members mode"""
    text = wrapped_fastq(111, 500000, lengths=(8000, 20000))
    cut = [0, 170001, 330003, len(text)]
    zipped = b"".join(gzip_sets.gz(text[a:b], flushes=[(p, zlib.Z_BLOCK) for p in range(3000, b - a, 3000)]) for a, b in zip(cut, cut[1:]))
    monkeypatch.setenv("CRASS_SHARD_MARGIN", "64")
    with ca.SearchGroup([0] * 3, local_copies=True) as g, ca.SearchEngine() as e:
        g.set_fastq_class(1)
        g.set_gzip_on_device(2, CHUNK)
        for r in range(3):
            g.rank_set_stage_timing(r, 1)
        sh = g.load_fastx_files([zipped])
        same_shards(sh, ca.fastx_files_shards_host_gzip([zipped], 3, fastq_class=1, gzip_mode=2, chunk_bytes=CHUNK), "wrapped")
        same_shards(sh, ca.fastx_files_shards_host([text], 3, fastq_class=1), "wrapped, the text")
        assert g.load_counters()[0] == 2 and g.load_counters()[2] > 0      # (the wrapped pass, with margin doublings)
        assert g.gzip_members_counters()[:2] == (1, 3)
        assert any(g.gzip_ms(r)["tail_windows"] > 0 for r in range(3))      # (the seeded walk ran, in members mode)
        got = records_of_group(g, sh.n_reads)
        e.set_fastq_class(1)
        e.set_gzip_on_device(True, members=True)
        assert_same_records(got, records_of_engine(e, [zipped]), "wrapped")


def test_a_damaged_member_declines_the_job(ca, groups):
    fa = gzip_sets.fasta(121, 40000)
    for n in (2, 3):
        g = groups(n)
        for name in ("crc_byte_of_member_1", "isize_of_member_2_off_by_one"):
            data, chunk, reason, member = DECLINED[name]
            assert chunk == CHUNK
            verdict = host_ranges(ca, "declined " + name, data, n)[0]
            assert verdict == (reason, member, OFFS[member])
            g.load_fastx_files(JOBS["paired"][0])       # something resident, so that the decline has something to take away
            with pytest.raises(ca.FastxFilesDeclined) as d:
                g.load_fastx_files([fa, data])
            want = ca.fastx_files_shards_host_gzip([fa, data], n, gzip_mode=2, chunk_bytes=CHUNK)
            assert d.value.status == 2 and d.value.layout.verdict == want.verdict == (1, 0, 0, verdict), (name, n, d.value.layout.verdict)
            with pytest.raises(ca.CrassError) as e:
                g.step()
            assert e.value.status == 6, name
