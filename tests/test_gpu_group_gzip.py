"""One plain gzip file inflated across the ranks of a group (crass_hip_group_inflate_gzip: k_gz_find / k_gz_count over each rank's
chunks, k_gz_decode / k_gz_windows_sym over its elements, the entry windows composed on the host, k_gz_window_resolve /
k_gz_narrow), and the files load that takes such files (crass_hip_group_set_gzip_on_device), against the host statements
(crass_gzip_inflate_ranges_host, crass_fastx_files_shards_host_gzip), the same load on the inflated files and the single
context's load with crass_hip_set_gzip_on_device.  Groups of 2, 3 and 4 contexts share device 0 (local copies), one group per
size; chunk 4096 throughout, so a file of a few hundred KB has tens of chain elements.  Every comparison is exact equality."""
import zlib

import numpy as np
import pytest

from tests import bgzf_sets, group_gzip_sets as ggs, gzip_sets

pytestmark = pytest.mark.gpu

REGULAR = gzip_sets.regular()
DECLINED = gzip_sets.declined()
CHUNK = ggs.CUT_CHUNK
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
    """one group per number of ranks, made on first use; `gz` groups have the switch on (chunk 4096), the others never had it set"""
    made = {}

    def get(n, gz=True):
        if (n, gz) not in made:
            made[(n, gz)] = ca.SearchGroup([0] * n, local_copies=True)
            if gz:
                made[(n, gz)].set_gzip_on_device(1, CHUNK)
        return made[(n, gz)]
    yield get
    for g in made.values():
        g.close()


@pytest.fixture(scope="module")
def eng(ca):
    with ca.SearchEngine() as e:
        e.set_gzip_on_device(True)
        yield e


def plan_tuple(p):
    return (p.n_chunks, p.n_chain, p.start_bit.tolist(), p.link.tolist(), p.text_len.tolist())


_host = {}


def host_ranges(ca, key, data, n, nominal=None):
    """crass_gzip_inflate_ranges_host's answer, once per file, number of ranges and cuts: (text, plan) or (verdict, plan)"""
    k = (key, n, None if nominal is None else tuple(nominal))
    if k not in _host:
        try:
            text, plan = ca.gzip_inflate_ranges_host(data, n, CHUNK, nominal=nominal, with_plan=True)
            _host[k] = (text, plan_tuple(plan))
        except ca.BgzfDeclined as e:
            _host[k] = (e.verdict, plan_tuple(e.plan))
    return _host[k]


def inflate_and_check(ca, g, key, data, nominal=None):
    want, want_plan = host_ranges(ca, key, data, g.n, nominal)
    what = (key, g.n, nominal)
    if isinstance(want, tuple):
        with pytest.raises(ca.BgzfDeclined) as e:
            g.inflate_gzip(data, CHUNK, nominal=nominal)
        assert e.value.status == 2 and e.value.verdict == want, (what, e.value.verdict, want)
        assert plan_tuple(e.value.plan) == want_plan, what
        return None
    got, plan = g.inflate_gzip(data, CHUNK, nominal=nominal, with_plan=True)
    assert len(got) == len(want), what
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%r: the text differs at %d places, first %d" % (what, len(bad), bad[0]))
    assert plan_tuple(plan) == want_plan, what
    return plan


# ---- 1. the distributed inflate ----
@pytest.mark.parametrize("n", SIZES)
def test_text_plan_and_verdict_are_the_host_functions(ca, groups, n):
    g = groups(n)
    assert set(gzip_sets.chained()) <= set(REGULAR) and {"short_blocks", "random_block_repeated"} <= set(REGULAR)
    for name in sorted(REGULAR):
        inflate_and_check(ca, g, name, REGULAR[name][0])
    for name in sorted(DECLINED):
        data, chunk, reason = DECLINED[name]
        assert chunk == CHUNK
        inflate_and_check(ca, g, "declined " + name, data)
        assert host_ranges(ca, "declined " + name, data, n)[0][0] == reason
    inflate_and_check(ca, g, "text_32769", REGULAR["text_32769"][0])      # (the group goes on behind a decline)


def held_elements(off, cuts):
    """the rule of gz_elements_for, restated: how many elements the ranges [cuts[r], cuts[r + 1]) hold, summed"""
    ends = np.asarray(off[1:], dtype=np.int64)
    n, total = len(ends), 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        e0 = 0 if a == 0 else int(np.searchsorted(ends, a, side="right"))
        e = int(np.searchsorted(ends, b, side="right"))
        if e < n and off[e] < b:
            e += 1
        total += e - e0
    return total


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["short_blocks", "random_block_repeated"])
def test_cuts_around_element_boundaries_empty_ranks_and_crowded_elements(ca, groups, name, n):
    g = groups(n)
    data, text = REGULAR[name]
    plan = ca.gzip_inflate_host(data, CHUNK, with_plan=True)[1]
    off = ggs.chain_offsets(plan)
    cuts = {k: v for k, v in ggs.boundary_cuts(off).items() if len(v) == n - 1}
    cuts.update(ggs.empty_and_crowded_cuts(off, n))
    assert len(cuts) >= 7
    for what, nominal in sorted(cuts.items()):
        inflate_and_check(ca, g, name, data, nominal)
        c = g.gzip_counters()
        # every element is narrowed by somebody, and the compressed bytes all went up
        assert c[:3] == (1, plan.n_chunks, plan.n_chain), (what, c)
        assert c[2] + c[3] == held_elements(off, [0] + list(nominal) + [off[-1]]), (what, c)
        assert c[4] >= len(data) - 18 and c[5] <= c[4], (what, c)
    nominal = ggs.empty_and_crowded_cuts(off, n)["crowded_in_one_element"]
    inflate_and_check(ca, g, name, data, nominal)
    assert g.gzip_counters()[3] >= n - 1            # (every rank holds that element)


def test_overflow_protocol_argument_errors_and_stage_times(ca, groups):
    import ctypes as C
    g = groups(3)
    data, text = REGULAR["fasta_level_9"]
    with pytest.raises(ca.CrassError) as e:
        g.inflate_gzip(data, CHUNK, out_cap=len(text) - 1)
    assert e.value.status == 8 and e.value.n_text == len(text) and not e.value.out.any()
    assert plan_tuple(e.value.plan) == host_ranges(ca, "fasta_level_9", data, 3)[1]
    a = np.frombuffer(data, np.uint8)
    n = C.c_uint64(0)
    out = np.zeros(len(text), np.uint8)
    f = g.lib.crass_hip_group_inflate_gzip
    assert f(g.h, a.ctypes.data, len(a), CHUNK, None, None, 0, C.byref(n), None, None) == 8 and n.value == len(text)
    assert f(None, a.ctypes.data, len(a), CHUNK, None, out.ctypes.data, len(out), C.byref(n), None, None) == 1
    assert f(g.h, None, len(a), CHUNK, None, out.ctypes.data, len(out), C.byref(n), None, None) == 1
    assert f(g.h, a.ctypes.data, len(a), CHUNK, None, out.ctypes.data, len(out), None, None, None) == 1
    assert f(g.h, a.ctypes.data, len(a), CHUNK, None, None, 5, C.byref(n), None, None) == 1
    for nominal in ([len(text) + 1, len(text) + 2], [5, 4]):
        nom = ggs.as_u64(nominal)
        assert f(g.h, a.ctypes.data, len(a), CHUNK, nom.ctypes.data, out.ctypes.data, len(out), C.byref(n), None, None) == 1, nominal
    assert not any(any(g.gzip_ms(r).values()) for r in range(3))
    for r in range(3):
        g.rank_set_stage_timing(r, 1)
    assert g.inflate_gzip(data, CHUNK).tobytes() == text
    for r in range(3):
        ms = g.gzip_ms(r)
        assert all(ms[k] > 0 for k in ("find", "count", "decode", "windows_sym", "narrow")) and ms["tail_windows"] == 0, (r, ms)
        g.rank_set_stage_timing(r, 0)


# ---- 2. the files load with the switch on ----
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
    """name -> (files as given, the same with every plain gzip file inflated)"""
    fq, fa, fq2 = gzip_sets.fastq(101, 300000), gzip_sets.fasta(102, 90000), gzip_sets.fastq(103, 120000)
    r1, r2 = gzip_sets.fastq(104, 200000), gzip_sets.fastq(105, 200000)
    blocked = bgzf_sets.bgzf(fq2, block=30011)
    # (a Z_BLOCK flush every few thousand text bytes: blocks shorter than a chunk, so the chain has tens of elements — zlib's own
    # blocks are 30 to 50 KB of input, a handful per file of this size; R2 is left as zlib writes it)
    flushed = lambda t, every, **kw: gzip_sets.gz(t, flushes=[(p, zlib.Z_BLOCK) for p in range(every, len(t), every)], **kw)
    return {"mixed": ([flushed(fq, 12000), fa, blocked], [fq, fa, blocked]),
            "paired": ([flushed(r1, 7000, level=1), gzip_sets.gz(r2, level=9)], [r1, r2])}


JOBS = jobs()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("job", sorted(JOBS))
def test_load_with_gzip_files_is_the_load_of_their_text(ca, groups, eng, job, n):
    g = groups(n)
    zipped, plain = JOBS[job]
    sh = g.load_fastx_files(zipped)
    same_shards(sh, ca.fastx_files_shards_host_gzip(zipped, n, gzip_mode=1, chunk_bytes=CHUNK), (job, n))
    c = g.gzip_counters()
    n_gz = sum(1 for z, p in zip(zipped, plain) if z is not p)
    assert c[0] == n_gz and c[2] >= 10 + n_gz and c[4] >= sum(len(z) - 18 for z, p in zip(zipped, plain) if z is not p), c
    got = records_of_group(g, sh.n_reads)
    g.load_fastx_files(plain)
    assert g.gzip_counters() == (0,) * 6                  # (no gzip file taken: BGZF is not one)
    assert_same_records(got, records_of_group(g, sh.n_reads), (job, n, "the same load on the text"))
    assert_same_records(got, records_of_engine(eng, zipped), (job, n, "one context, gzip on device"))
    g.load_fastx_files(zipped)
    g.step()                                              # (the search path runs on what was loaded)


def test_cuts_that_leave_ranks_empty(ca, groups):
    zipped, plain = JOBS["mixed"]
    T = len(plain[0]) + len(plain[1]) + len(gzip_sets.fastq(103, 120000))      # (the job's text space: the BGZF file by its text)
    want = None
    for n, nominal in ((3, [0, 0]), (3, [T, T]), (4, [1000, 1000, 1001]), (4, [len(plain[0]), len(plain[0]), len(plain[0]) + 5])):
        g = groups(n)
        sh = g.load_fastx_files(zipped, nominal=nominal)
        same_shards(sh, ca.fastx_files_shards_host_gzip(zipped, n, nominal=nominal, gzip_mode=1, chunk_bytes=CHUNK), (n, nominal))
        got = records_of_group(g, sh.n_reads)
        if want is None:
            g.load_fastx_files(plain, nominal=nominal)
            want = records_of_group(g, sh.n_reads)
        assert_same_records(got, want, (n, nominal))


def wrapped_fastq(seed, n_bytes, width=60, lengths=(100, 400)):
    rng = np.random.RandomState(seed)
    recs, size, i = [], 0, 0
    while size < n_bytes:
        L = int(rng.randint(*lengths))
        s = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, L)].tobytes()
        q = np.frombuffer(b"FFFF@:,#+F", np.uint8)[rng.randint(0, 10, L)].tobytes()      # ('@' and '+' at line starts too)
        wrap = lambda x: b"\n".join(x[k:k + width] for k in range(0, L, width))
        r = b"@w%d c%d\n%s\n+\n%s\n" % (i, i % 3, wrap(s), wrap(q))
        recs.append(r); size += len(r); i += 1
    return b"".join(recs)


def test_wrapped_fastq_in_a_gzip_file(ca, monkeypatch):
    # records of 16 to 40 KB, several chain elements each (an element is about 12 KB of this text at a chunk of 4096 bytes): a margin
    # of 64 bytes that doubles until a record ends has the rank pull further elements, one seeded walk per doubling that needs some
    text = wrapped_fastq(111, 500000, lengths=(8000, 20000))
    zipped = gzip_sets.gz(text, flushes=[(p, zlib.Z_BLOCK) for p in range(3000, len(text), 3000)])
    monkeypatch.setenv("CRASS_SHARD_MARGIN", "64")
    with ca.SearchGroup([0] * 3, local_copies=True) as g, ca.SearchEngine() as e:
        g.set_fastq_class(1)
        g.set_gzip_on_device(1, CHUNK)
        for r in range(3):
            g.rank_set_stage_timing(r, 1)
        sh = g.load_fastx_files([zipped])
        same_shards(sh, ca.fastx_files_shards_host_gzip([zipped], 3, fastq_class=1, gzip_mode=1, chunk_bytes=CHUNK), "wrapped")
        same_shards(sh, ca.fastx_files_shards_host([text], 3, fastq_class=1), "wrapped, the text")
        assert g.load_counters()[0] == 2 and g.load_counters()[2] > 0      # (the wrapped pass, with margin doublings)
        # the margin growth pulled further elements through the seeded window walk: more elements were inflated by a further rank
        # than the ranks' nominal pieces hold, and the walk's kernel was timed on some rank
        c = g.gzip_counters()
        plan = ca.gzip_inflate_host(zipped, CHUNK, with_plan=True)[1]
        off = ggs.chain_offsets(plan)
        cuts = [len(text) * k // 3 for k in range(4)]
        nominal_held = held_elements(off, [0] + [x - 1 for x in cuts[1:3]] + [cuts[3]])      # (an upper bound: pieces with the byte in front)
        assert c[:3] == (1, plan.n_chunks, plan.n_chain) and plan.n_chain > 10, c
        assert c[2] + c[3] > nominal_held + 1, (c, nominal_held)
        assert any(g.gzip_ms(r)["tail_windows"] > 0 for r in range(3))
        got = records_of_group(g, sh.n_reads)
        e.set_fastq_class(1)
        e.set_gzip_on_device(True)
        assert_same_records(got, records_of_engine(e, [zipped]), "wrapped")


# ---- 3. the switch off, damaged files, several members ----
def test_switch_off_is_the_decline_of_before(ca, groups):
    g = groups(2, gz=False)
    for job in sorted(JOBS):
        zipped, plain = JOBS[job]
        with pytest.raises(ca.FastxFilesDeclined) as d:
            g.load_fastx_files(zipped)
        assert d.value.status == 2 and d.value.layout.verdict == (0, 0, 0, (gzip_sets.NOT_BGZF, 0, 0))
        assert d.value.layout.verdict == ca.fastx_files_shards_host(zipped, 2).verdict == ca.fastx_files_shards_host_gzip(zipped, 2, gzip_mode=0).verdict
        with pytest.raises(ca.CrassError) as e:
            g.step()
        assert e.value.status == 6
    blocked = JOBS["mixed"][0][2]
    g.load_fastx_files([blocked])
    assert g.gzip_counters() == (0,) * 6
    # ... and on, then off again, on the same group
    g3 = groups(3)
    g3.set_gzip_on_device(0)
    with pytest.raises(ca.FastxFilesDeclined) as d:
        g3.load_fastx_files(JOBS["paired"][0])
    assert d.value.layout.verdict == (0, 0, 0, (gzip_sets.NOT_BGZF, 0, 0))
    g3.set_gzip_on_device(1, CHUNK)
    assert g3.load_fastx_files(JOBS["paired"][0]).accepted


def flips_by_kind(ca):
    """three flipped copies of gzip_sets.flip_file(): one a run of a chunk behind the first declines (the chain knows it), one with
    a wrong CRC-32, one with an unresolved marker.  The 200 flips of bit_flips() hold no marker case (a distance that reaches in
    front of the text is rare): that one is the first of bit_flips(1000)"""
    out = {}
    for flips in (gzip_sets.bit_flips(), gzip_sets.bit_flips(1000)):
        for i, data in enumerate(flips):
            try:
                ca.gzip_inflate_host(data, CHUNK)
            except ca.BgzfDeclined as e:
                kind = "crc" if e.reason == gzip_sets.CRC else "marker" if e.reason == gzip_sets.MARKER else "chain" if 1 <= e.reason <= 6 and e.member > 0 else None
                if kind and kind not in out:
                    out[kind] = (i, data, e.verdict)
            if len(out) == 3:
                return out
    return out


def test_damaged_and_several_member_files_decline_the_job(ca, groups):
    assert gzip_sets.FLIP_CHUNK == CHUNK
    flips = flips_by_kind(ca)
    assert sorted(flips) == ["chain", "crc", "marker"], sorted(flips)
    fa = gzip_sets.fasta(121, 40000)
    cases = [(k, data, v) for k, (i, data, v) in sorted(flips.items())]
    two = DECLINED["two_members"][0]
    cases.append(("two_members", two, host_ranges(ca, "declined two_members", two, 2)[0]))
    assert cases[-1][2][0] == gzip_sets.TRAILING == 13
    for n in (2, 3):
        g = groups(n)
        for kind, data, verdict in cases:
            g.load_fastx_files(JOBS["paired"][0])       # something resident, so that the decline has something to take away
            with pytest.raises(ca.FastxFilesDeclined) as d:
                g.load_fastx_files([fa, data])
            want = ca.fastx_files_shards_host_gzip([fa, data], n, gzip_mode=1, chunk_bytes=CHUNK)
            assert d.value.status == 2 and d.value.layout.verdict == want.verdict == (1, 0, 0, verdict), (kind, n, d.value.layout.verdict)
            with pytest.raises(ca.CrassError) as e:
                g.step()
            assert e.value.status == 6, kind
