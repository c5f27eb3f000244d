"""Wrapped FASTQ across the ranks of a group (crass_hip_group_set_fastq_class + crass_hip_group_load_fastx_files): shards cut at the
records REACHABLE from a file's line 0 (k_fw_cut_next / k_fw_cut_jump / k_fw_cut_lookup and the chain over the ranks), against the
host statement of the rule (crass_fastx_files_shards_host_class) and the single context's class-1 load: the shards, every read's
text, header line and quality, the counters of the load, the verdict of every offending input, and the whole search path.  N
contexts share device 0 (local copies); one group per N is reused across the loads.  Every comparison is exact equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import orc, shard_sets, shard_wrapped_sets as S, wrapped_sets
from tests.parity import assert_same_pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = S.cases()
DECLINED = S.declined()
SWEPT = {"decoy": S.DECOY, "second": S.second_small()}
GROWN = ("mixed_job", "record_longer_than_a_range")


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    assert crass_amd.load().crass_hip_fastx_tile_bytes() == S.TILE
    return crass_amd


@pytest.fixture(scope="module")
def eng(ca):
    with ca.SearchEngine() as e:
        e.set_fastq_class(1)
        yield e


@pytest.fixture(scope="module")
def groups(ca):
    """one class-1 group per number of ranks, made on first use: creating contexts is the expensive part"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = ca.SearchGroup([0] * n, local_copies=True)
            made[n].set_fastq_class(1)
        return made[n]
    yield get
    for g in made.values():
        g.close()


def single(eng, files):
    """what the single context gives on the files under its class: every read's text, header line and quality"""
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


def assert_same_shards(ca, sh, files, n, nominal, what, fastq_class=1):
    host = ca.fastx_files_shards_host(files, n, nominal, fastq_class=fastq_class)
    assert sh.accepted and host.accepted, what
    assert (sh.n_ranks, sh.n_files, sh.n_reads, sh.max_len, sh.formats) == (host.n_ranks, host.n_files, host.n_reads, host.max_len, host.formats), what
    assert sh.cuts == host.cuts, (what, sh.cuts, host.cuts)
    for k in ("rank_read_base", "file_read_base"):
        assert np.array_equal(getattr(sh, k), getattr(host, k)), (what, k, getattr(sh, k), getattr(host, k))


# ---- (a) the nominal cut swept over every byte ----
def sweep(ca, eng, g, name):
    """every byte of the file as the nominal cut on 2 ranks; returns the margin doublings of all loads"""
    files = [SWEPT[name]]
    want = single(eng, files)
    starts = S.record_starts(files[0])
    assert want["n"] == len(starts)
    seen, doublings = set(), 0
    for x in range(len(files[0]) + 1):
        sh = g.load_fastx_files(files, nominal=[x])
        assert_same_shards(ca, sh, files, 2, [x], (name, x))
        cnt = g.load_counters()
        assert cnt[0] == 2 and cnt[1] == 1 and cnt[3] >= 1, (name, x, cnt)
        doublings += cnt[2]
        seen.add(sh.cuts[1])
        assert_same_records(g, want, (name, x))
    assert seen == {(0, p) for p in starts} | {(1, 0)}      # every record start was a cut, and the end — and nothing else
    return doublings


@pytest.mark.parametrize("name", sorted(SWEPT))
def test_every_byte_as_the_nominal_cut(ca, eng, groups, name):
    assert "CRASS_SHARD_MARGIN" not in os.environ
    assert sweep(ca, eng, groups(2), name) == 0          # (the default margin holds these files whole)
    if name == "decoy":
        for x in range(41, 61):                          # never the decoy at 60
            assert groups(2).load_fastx_files([S.DECOY], nominal=[x]).cuts[1] == (0, 77)


def run_sweeps():
    """the same sweeps in a process of their own (test_every_byte_with_a_tiny_margin sets CRASS_SHARD_MARGIN for it)"""
    import crass_amd as ca
    ca.load()
    with ca.SearchEngine() as eng, ca.SearchGroup([0, 0], local_copies=True) as g:
        eng.set_fastq_class(1)
        g.set_fastq_class(1)
        for name in sorted(SWEPT):
            print("sweep ok %s doublings %d" % (name, sweep(ca, eng, g, name)), flush=True)
        # a margin that doubles many times (a read of 9 000 bases), and one that grows by BGZF members
        with ca.SearchGroup([0, 0, 0], local_copies=True) as g3:
            g3.set_fastq_class(1)
            for name in GROWN:
                files, positions, n_chained = CASES[name]
                want = single(eng, files)
                doublings = 0
                for n, grp in ((2, g), (3, g3)):
                    for nominal in S.nominal_lists(files, positions, n):
                        sh = grp.load_fastx_files(files, nominal=nominal)
                        assert_same_shards(ca, sh, files, n, nominal, (name, n, nominal))
                        assert grp.load_counters()[:2] == (2, n_chained)
                        doublings += grp.load_counters()[2]
                        assert_same_records(grp, want, (name, n, nominal))
                print("grown ok %s doublings %d" % (name, doublings), flush=True)


def test_every_byte_with_a_tiny_margin(ca):
    """CRASS_SHARD_MARGIN=16 in a fresh process: a record that begins in a piece seldom ends within 16 bytes of the piece's end, so
    the chain is unresolved there and the rank doubles its margin until it is not"""
    code = "from tests.test_gpu_group_wrapped_files import run_sweeps\nrun_sweeps()\n"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, CRASS_SHARD_MARGIN="16"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("sweep ok ")]
    assert [ln[2] for ln in lines] == sorted(SWEPT), r.stdout[-2000:]
    assert all(int(ln[4]) > 0 for ln in lines), lines
    grown = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("grown ok ")]
    assert [ln[2] for ln in grown] == list(GROWN) and all(int(ln[4]) > 0 for ln in grown), r.stdout[-2000:]


# ---- (b) the designed jobs ----
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_designed_jobs(ca, eng, groups, name, n):
    files, positions, n_chained = CASES[name]
    want = single(eng, files)
    g = groups(n)
    for nominal in S.nominal_lists(files, positions, n):
        sh = g.load_fastx_files(files, nominal=nominal)
        assert_same_shards(ca, sh, files, n, nominal, (name, n, nominal))
        cnt = g.load_counters()
        assert cnt[0] == 2 and cnt[1] == n_chained, (name, n, nominal, cnt)
        assert_same_records(g, want, (name, n, nominal))
        assert [g.rank_counters(r)["n_reads"] for r in range(n)] == np.diff(sh.rank_read_base).tolist(), (name, n, nominal)
    if name in ("record_longer_than_a_range", "more_ranks_than_records") and n == 4:
        assert 0 in np.diff(g.load_fastx_files(files).rank_read_base).tolist()      # an empty rank


# ---- (c) a four-line job pays nothing ----
def test_a_four_line_job_takes_one_attempt(ca, groups):
    files = S.four_line_job()
    with ca.SearchEngine() as e0, ca.SearchGroup([0, 0, 0], local_copies=True) as g0:      # class 0: the switch never set
        want = single(e0, files)
        for nominal in (None, [100, 700], [0, len(files[0])]):
            sh0 = g0.load_fastx_files(files, nominal=nominal)
            assert g0.load_counters() == (1, 0, 0, 0)
            g = groups(3)
            sh = g.load_fastx_files(files, nominal=nominal)
            assert g.load_counters() == (1, 0, 0, 0), nominal
            assert_same_shards(ca, sh, files, 3, nominal, nominal, fastq_class=0)
            assert sh.cuts == sh0.cuts and np.array_equal(sh.rank_read_base, sh0.rank_read_base)
            assert_same_records(g, want, nominal)
            for r in range(3):
                four, wrapped = g.rank_last_scan_classes(r)
                assert wrapped == 0 and (four, wrapped) == g0.rank_last_scan_classes(r), (nominal, r)


# ---- (d) offending inputs ----
@pytest.mark.parametrize("name", sorted(DECLINED))
def test_offending_inputs(ca, groups, name):
    files, positions = DECLINED[name]
    want = ca.fastx_files_scan_host(files, fastq_class=1)
    assert not want.accepted
    good = [S.DECOY]
    for n in (2, 3):
        g = groups(n)
        for nominal in S.nominal_lists(files, positions, n):
            host = ca.fastx_files_shards_host(files, n, nominal, fastq_class=1)
            assert host.verdict == want.verdict
            assert g.load_fastx_files(good).n_reads == 4                 # (reads are resident before the declined load)
            with pytest.raises(ca.FastxFilesDeclined) as e:
                g.load_fastx_files(files, nominal=nominal)
            assert e.value.status == 2 and e.value.layout.verdict == want.verdict, (name, n, nominal, e.value.layout.verdict, want.verdict)
            assert len(e.value.layout.rank_read_base) == 0
            assert 1 <= g.load_counters()[0] <= 2
            with pytest.raises(ca.CrassError) as st:
                g.step()
            assert st.value.status == 6
            with pytest.raises(ca.CrassError) as st:
                g.fetch_header_lines([0])
            assert st.value.status == 6
            assert all(g.rank_counters(r)["n_reads"] == 0 for r in range(n))


# ---- (e) the switch off ----
def test_class_0_declines_as_before(ca):
    with ca.SearchGroup([0, 0], local_copies=True) as g:
        for setting in (None, 1, 0):
            if setting is not None:
                g.set_fastq_class(setting)
            for name in ("decoy", "crlf", "mixed_job"):
                files, positions, _ = CASES[name]
                want = ca.fastx_files_shards_host(files, 2)              # the four-line rule's verdict
                assert not want.accepted and want.verdict == ca.fastx_files_scan_host(files).verdict
                for nominal in S.nominal_lists(files, positions, 2)[:3]:
                    if setting == 1:
                        assert g.load_fastx_files(files, nominal=nominal).accepted
                        continue
                    with pytest.raises(ca.FastxFilesDeclined) as e:
                        g.load_fastx_files(files, nominal=nominal)
                    assert e.value.layout.verdict == want.verdict, (setting, name, nominal)
                    assert g.load_counters() == (1, 0, 0, 0)
                    assert all(g.rank_counters(r)["n_reads"] == 0 for r in range(2))
        with pytest.raises(ca.CrassError) as e:
            g.set_fastq_class(2)
        assert e.value.status == 1


# ---- (f) the whole path ----
def test_the_whole_path_on_a_wrapped_paired_job(ca, eng, groups):
    n, L = 12000, 150
    spec = ca.synth_spec(read_len=L, crispr_per_million=60000, n_dr=8)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    rng = np.random.default_rng(29)
    recs = []
    for i in range(n):
        s = asc[i * L:(i + 1) * L].tobytes()
        if i % 11 == 0:
            s = s[:int(rng.integers(70, L))]
        # every 3rd read: the name of a read anywhere in the job, in either file (that read, 1 modulo 3, keeps its own name)
        recs.append((b"r%d" % (i if i % 3 else (7 * i + 1) % n), s))
    wrapped = lambda part, k0: b"".join(wrapped_sets.wfq(nm + (b" c" + nm if (k0 + k) % 4 else b""), s, bytes(64 + (k + i) % 60 for i in range(len(s))), w=60,
                                                        after=(b"",) if k % 7 == 0 else ()) for k, (nm, s) in enumerate(part))
    h = n // 2
    files = [wrapped(recs[:h], 0), wrapped(recs[h:], h)]
    seqs, hdrs = [s for _, s in recs], [nm for nm, _ in recs]
    ref = orc.pipeline(seqs, hdrs)
    lay = eng.load_fastx_files(files)
    assert lay.n_reads == n
    want_comments = eng.fetch_comments(np.arange(n, dtype=np.uint64))
    for k in (2, 3):
        g = groups(k)
        sh = g.load_fastx_files(files)
        assert g.load_counters()[:2] == (2, 2)
        assert_same_shards(ca, sh, files, k, None, k)
        assert sh.n_reads == n and np.all(np.diff(sh.rank_read_base) > 0)
        g.step()
        grp = g.result()
        assert_same_pipeline(grp, ref)
        got = g.fetch_comments(np.arange(n, dtype=np.uint64))
        assert np.array_equal(got[1], want_comments[1]) and np.array_equal(got[2], want_comments[2])
        assert np.array_equal(got[0][:int(got[1][-1])], want_comments[0][:int(want_comments[1][-1])])
        pick = grp.rec_read[::max(1, len(grp.rec_read) // 50)]
        chars, off, name_len = g.fetch_header_lines(pick)
        for j, r in enumerate(pick):
            nm = recs[int(r)][0]
            assert bytes(chars[int(off[j]):int(off[j + 1])]).split(b" ")[0] == nm and int(name_len[j]) == len(nm)
    assert orc.pipeline(seqs).n_pass2 > ref.n_pass2      # the cross-rank suppression is shown to act
