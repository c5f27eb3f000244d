"""Device ingest across the ranks of a group (crass_hip_group_load_fastx_files): record-aligned shards of the files' bytes, cut on
the device (k_fx_cut_probe), against the host statement of the cut rule (crass_fastx_files_shards_host) and the single context's
files load (crass_hip_load_fastx_files): the shards, every read's text, header line and quality, the verdict of a declined input,
and the whole search path with names that repeat across ranks.  N contexts share device 0 (local copies); one group per N is
reused across the loads.  Every comparison is exact equality."""
import numpy as np
import pytest

from tests import bgzf_sets, files_sets, orc, shard_sets
from tests.parity import assert_same_pipeline

pytestmark = pytest.mark.gpu

CASES = shard_sets.cases()
DECLINED = dict(shard_sets.declined(), **{k: (v[0], [None]) for k, v in files_sets.declined().items()})


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    assert crass_amd.load().crass_hip_fastx_tile_bytes() == shard_sets.TILE
    return crass_amd


@pytest.fixture(scope="module")
def eng(ca):
    with ca.SearchEngine() as e:
        yield e


@pytest.fixture(scope="module")
def groups(ca):
    """one group per number of ranks, made on first use: creating contexts is the expensive part"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = ca.SearchGroup([0] * n, local_copies=True)
        return made[n]
    yield get
    for g in made.values():
        g.close()


def single(eng, files):
    """what the single context gives on the files: every read's text, header line (with the name's length) and quality"""
    lay = eng.load_fastx_files(files)
    idx = np.arange(lay.n_reads, dtype=np.uint64)
    t = eng.fetch_text(idx)
    addr, nb = eng.resident_fastx()
    hl = eng.fetch_header_lines(addr, np.append(lay.rec_pos[:-1], nb), idx)
    ql = eng.fetch_quality(addr, nb, lay.rec_pos, idx)
    return {"n": lay.n_reads, "text": (t.chars.copy(), t.off.copy()), "lines": hl, "quality": ql}


def assert_same_records(g, want, what):
    n = want["n"]
    idx = np.arange(n, dtype=np.uint64)
    t = g.fetch_text(idx)
    assert np.array_equal(t.off, want["text"][1]) and np.array_equal(t.chars[:int(t.off[-1])], want["text"][0][:int(t.off[-1])]), (what, "text")
    for got, ref, k in ((g.fetch_header_lines(idx), want["lines"], "lines"), (g.fetch_quality(idx), want["quality"], "quality")):
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0][:int(got[1][-1])], ref[0][:int(ref[1][-1])]), (what, k)
        assert np.array_equal(got[2], ref[2]), (what, k, "second")
    if n > 2:                                           # any order, repeats
        pick = np.array([n - 1, 0, n // 2, 0], dtype=np.uint64)
        # header lines with their name lengths, quality strings with has_qual: each against the single context's for that record
        for got, ref, k in ((g.fetch_header_lines(pick), want["lines"], "lines"), (g.fetch_quality(pick), want["quality"], "quality")):
            assert len(got[1]) == len(pick) + 1 and len(got[2]) == len(pick), (what, k)
            for j, r in enumerate(pick):
                r = int(r)
                assert bytes(got[0][int(got[1][j]):int(got[1][j + 1])]) == bytes(ref[0][int(ref[1][r]):int(ref[1][r + 1])]), (what, k, j)
                assert got[2][j] == ref[2][r], (what, k, j, "second")


def assert_same_shards(ca, sh, files, n, nominal, what):
    host = ca.fastx_files_shards_host(files, n, nominal)
    assert sh.accepted and host.accepted, what
    assert (sh.n_ranks, sh.n_files, sh.n_reads, sh.max_len, sh.formats) == (host.n_ranks, host.n_files, host.n_reads, host.max_len, host.formats), what
    assert sh.cuts == host.cuts, (what, sh.cuts, host.cuts)
    for k in ("rank_read_base", "file_read_base"):
        assert np.array_equal(getattr(sh, k), getattr(host, k)), (what, k, getattr(sh, k), getattr(host, k))


# ---- (a) the nominal cut swept over every byte ----
@pytest.mark.parametrize("name", ["fastq", "fasta"])
def test_every_byte_as_the_nominal_cut(ca, eng, groups, name):
    files = [shard_sets.small_fastq() if name == "fastq" else shard_sets.small_fasta()]
    want = single(eng, files)
    g = groups(2)
    seen = set()
    for x in range(len(files[0]) + 1):
        sh = g.load_fastx_files(files, nominal=[x])
        assert_same_shards(ca, sh, files, 2, [x], (name, x))
        seen.add(sh.cuts[1])
        assert_same_records(g, want, (name, x))
    assert len(seen) == want["n"] + 1                    # every record start was a cut, and the end


# ---- (b) the designed cases ----
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_designed_cases(ca, eng, groups, name, n):
    files, positions = CASES[name]
    want = single(eng, files)
    g = groups(n)
    for nominal in shard_sets.nominal_lists(files, positions, n):
        sh = g.load_fastx_files(files, nominal=nominal)
        assert_same_shards(ca, sh, files, n, nominal, (name, n, nominal))
        assert_same_records(g, want, (name, n, nominal))
        cnt = [g.rank_counters(r)["n_reads"] for r in range(n)]
        assert cnt == np.diff(sh.rank_read_base).tolist(), (name, n, nominal)
    if name in ("record_longer_than_a_range", "more_ranks_than_records") and n == 4:
        sh = g.load_fastx_files(files)
        assert 0 in np.diff(sh.rank_read_base).tolist()  # an empty rank


def test_the_probe_on_every_alignment_and_on_tile_edges(ca, eng):
    """k_fx_cut_probe itself against the serial probe: ranges of a few tiles that start at every alignment 0 .. 15, end on and
    around tile and vector edges, with and without a line start at their first byte; several blocks' parts folded"""
    import torch
    rng = np.random.default_rng(5)
    text = shard_sets.tile_edge_fastq(shard_sets.TILE, __import__("random").Random(3)) * 3
    arr = np.frombuffer(text, np.uint8).copy()
    # lines of every length around 16, '>' at line starts and inside lines
    extra = bytearray()
    for k in range(600):
        extra += (b">" if k % 3 == 0 else b"A") + bytes(rng.integers(65, 90, size=int(rng.integers(0, 40))).astype(np.uint8)) + (b">" if k % 5 == 0 else b"") + b"\n"
    arr = np.concatenate([arr, np.frombuffer(bytes(extra), np.uint8)])
    dev = torch.zeros(len(arr) + 64, dtype=torch.uint8, device="cuda")
    for lead in range(16):
        dev[lead:lead + len(arr)] = torch.from_numpy(arr).cuda()
        torch.cuda.synchronize()
        base = int(dev.data_ptr()) + lead
        assert base % 16 == lead
        T = shard_sets.TILE
        for a, b in ((0, len(arr)), (1, T), (T - lead, 2 * T - lead), (T - lead - 1, 2 * T - lead + 1), (5, 5), (7, 8), (len(text), len(arr)),
                     (len(text) + 3, len(text) + 16 + lead), (2 * T + 1, 3 * T + 17)):
            for left in (False, True):
                want = ca.fastx_cut_probe_host(arr[a:b].tobytes(), left)
                got = eng.cut_probe_device(base + a, b - a, left)
                assert np.array_equal(got, want), (lead, a, b, left, got, want)
    # more tiles than blocks: a block walks several tiles in order
    big = np.tile(arr, 200)[:5000 * 1000]
    dbig = torch.from_numpy(big).cuda()
    torch.cuda.synchronize()
    for a in (0, 3, 4099):
        want = ca.fastx_cut_probe_host(big[a:].tobytes(), a == 0)
        got = eng.cut_probe_device(int(dbig.data_ptr()) + a, len(big) - a, a == 0)
        assert np.array_equal(got, want), a


# ---- (c) declined inputs ----
@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_inputs(ca, groups, name):
    files, positions = DECLINED[name]
    want = ca.fastx_files_scan_host(files)
    assert not want.accepted
    good = [shard_sets.small_fasta()]
    for n in (2, 3):
        g = groups(n)
        for nominal in shard_sets.nominal_lists(files, positions, n):
            g.load_fastx_files(good)                     # (reads are resident before the declined load)
            with pytest.raises(ca.FastxFilesDeclined) as e:
                g.load_fastx_files(files, nominal=nominal)
            assert e.value.status == 2 and e.value.layout.verdict == want.verdict, (name, n, nominal, e.value.layout.verdict, want.verdict)
            assert len(e.value.layout.rank_read_base) == 0
            with pytest.raises(ca.CrassError) as st:
                g.step()
            assert st.value.status == 6
            with pytest.raises(ca.CrassError) as st:
                g.fetch_header_lines([0])
            assert st.value.status == 6
            assert all(g.rank_counters(r)["n_reads"] == 0 for r in range(n))


# ---- (d) the whole path ----
@pytest.fixture(scope="module")
def records(ca):
    """30 000 synthetic reads of up to 150 bases: ragged lengths, N reads, names that repeat inside a file and across the two"""
    n, L = 30000, 150
    spec = ca.synth_spec(read_len=L, crispr_per_million=60000, n_dr=8)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    rng = np.random.default_rng(15)
    out = []
    for i in range(n):
        s = asc[i * L:(i + 1) * L].tobytes()
        if i % 11 == 0:
            s = s[:int(rng.integers(70, L))]
        if i % 501 == 0:
            s = s[:40] + b"N" + s[41:]
        # every 3rd read: the name of a read anywhere in the job, in either file (that read, 1 modulo 3, keeps its own name)
        out.append((b"r%d" % (i if i % 3 else (7 * i + 1) % n), s))
    return out


def fq_of(recs):
    return b"".join(b"@" + nm + b" c" + nm + b"\n" + s + b"\n+\n" + bytes(70 + (k + i) % 40 for i in range(len(s))) + b"\n" for k, (nm, s) in enumerate(recs))


@pytest.mark.parametrize("kind", ["two_fastq", "bgzf"])
def test_the_whole_path(ca, eng, groups, records, kind):
    h = len(records) // 2
    files = [fq_of(records[:h]), fq_of(records[h:])]
    if kind == "bgzf":
        files = [bgzf_sets.bgzf(files[0]), bgzf_sets.bgzf(files[1], block=20000)]
    seqs, hdrs = [s for _, s in records], [nm for nm, _ in records]
    ref = orc.pipeline(seqs, hdrs)
    eng.load_fastx_files(files)
    cand, merge = eng.seed_scan(), eng.merge()
    rec = eng.recruit()
    one = ca.engine.PipelineResult(cand, eng.merge_view(), rec, cand.max_read_len)
    assert_same_pipeline(one, ref)
    for n in (2, 3):
        g = groups(n)
        sh = g.load_fastx_files(files)
        assert sh.n_reads == len(records) and np.all(np.diff(sh.rank_read_base) > 0)
        g.step()
        grp = g.result()
        assert_same_pipeline(grp, ref)
        np.testing.assert_array_equal(grp.rec_read, one.rec_read)
        np.testing.assert_array_equal(grp.rec_token, one.rec_token)
        assert grp.tokens == one.tokens and grp.groups == one.groups and grp.patterns == one.patterns
        g.step()                                         # (a second step on the same load: the names are exchanged again)
        assert_same_pipeline(g.result(), ref)
        # the handed-on records' lines from the ranks' arenas
        pick = grp.rec_read[::max(1, len(grp.rec_read) // 50)]
        chars, off, name_len = g.fetch_header_lines(pick)
        for j, r in enumerate(pick):
            nm = records[int(r)][0]
            assert bytes(chars[int(off[j]):int(off[j + 1])]) == nm + b" c" + nm and int(name_len[j]) == len(nm)
    # the cross-rank suppression is shown to act: without headers more reads are recruited
    assert orc.pipeline(seqs).n_pass2 > ref.n_pass2


# ---- (e) entry points ----
def test_a_group_of_one_rank_equals_the_single_context(ca, eng, groups):
    files = CASES["fasta_fastq_bgzf"][0]
    want = single(eng, files)
    g = groups(1)
    sh = g.load_fastx_files(files)
    assert_same_shards(ca, sh, files, 1, None, "one rank")
    assert sh.cuts == [(0, 0), (len(files), 0)] and sh.rank_read_base.tolist() == [0, want["n"]]
    assert_same_records(g, want, "one rank")
    a, b = g.rank_counters(0), eng.counters()
    assert (a["n_reads"], a["n_exceptions"]) == (b["n_reads"], b["n_exceptions"])


def test_the_line_fetches_need_a_files_load(ca, groups):
    g = groups(2)
    g.load_fastx_files([shard_sets.small_fastq()])
    assert g.fetch_quality([0])[2].tolist() == [1]
    seqs = [b"ACGTACGTACGTACGTACGT" * 3] * 8
    packed = ca.PackedReads(seqs)
    g.load_reads(packed)
    for fetch in (g.fetch_header_lines, g.fetch_quality):
        with pytest.raises(ca.CrassError) as e:
            fetch([0])
        assert e.value.status == 6
    assert g.fetch_text([0])[0] == seqs[0]
    packed.close()
    with pytest.raises(ValueError):
        g.load_fastx_files([shard_sets.small_fastq()], nominal=[5, 6])      # (n - 1 cuts)
    with pytest.raises(ca.CrassError) as e:
        g.load_fastx_files([shard_sets.small_fastq()], pad_uniform=3)
    assert e.value.status == 1
