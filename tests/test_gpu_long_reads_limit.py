"""Every read the library loads is searched: sets whose longest read has 28 001 .. 60 000 bases (the last-resort launch of the
survivor kernel with rows for max(highDR, highSp) bases, survivor_lds_last_resort) through the search, its route switches, a
group of two contexts, the text fetch, the consensus stage and the command line — against the oracle on the designed reads of
tests/long_limit_sets.py (test_long_limit_sets_host.py pins the oracle's answer to the design).  Every comparison is exact.

Before the bounded rows, the first seed_scan of each of these sets — all but the one whose longest read has L_OK bases — answered
CRASS_ERR_UNSUPPORTED (status 2)."""
import os
import subprocess

import numpy as np
import pytest

from tests import orc, long_limit_sets as S
from tests.parity import assert_same_pipeline

pytestmark = pytest.mark.gpu

DRAWS = {"defaults": {}, "w7_d20_D40": dict(searchWindowLength=7, lowDRsize=20, highDRsize=40)}
SWITCHES = ["CRASS_LONG_FULL_LAYOUT", "CRASS_NO_LIGHT", "CRASS_SEQ_WINDOW", "CRASS_ROW_CAP"]
STAMP = "01_01_2026_000000"


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


_refs = {}


def seqs_up_to(max_len=S.MAX_READ_LEN):
    return [r.seq for r in S.subset_up_to(S.get(), max_len)]


def reference(draw="defaults", max_len=S.MAX_READ_LEN):
    """the oracle's answer, computed once per draw and set and shared"""
    if (draw, max_len) not in _refs:
        _refs[(draw, max_len)] = orc.pipeline(seqs_up_to(max_len), params=orc.Params.default(**DRAWS[draw]))
    return _refs[(draw, max_len)]


def assert_not_empty(ref, max_len=S.MAX_READ_LEN):
    reads = S.subset_up_to(S.get(), max_len)
    assert ref.n_pass1 == sum(1 for r in reads if r.dr) > 0 and ref.n_pass2 > 0


@pytest.mark.parametrize("draw", sorted(DRAWS))
def test_the_set_through_search_pipeline(ca, draw):
    ref = reference(draw)
    assert_not_empty(ref)
    gpu = ca.search_pipeline(seqs_up_to(), params=ca.default_params(**DRAWS[draw]))
    assert_same_pipeline(gpu, ref)
    assert gpu.max_read_len == S.MAX_READ_LEN
    assert gpu.n_pass1 == 8 and gpu.n_pass2 == 4 and max(int(x) for x in gpu.ss_pool) == S.MAX_READ_LEN - 1


@pytest.mark.parametrize("max_len", [S.L_OK, S.L_OK + 1, 40952, 40953, 59999])
def test_a_set_whose_longest_read_sits_at_a_boundary_of_the_layout(ca, max_len):
    """L_OK: the last set with rows of the read's own length (the layout as it always was); L_OK + 1: the first with bounded rows;
    40 952 / 40 953: the rows alone reach 160 KB; 59 999: one below the ceiling (60 000: the test above)"""
    ref = reference("defaults", max_len)
    assert_not_empty(ref, max_len)
    gpu = ca.search_pipeline(seqs_up_to(max_len))
    assert_same_pipeline(gpu, ref)
    assert gpu.max_read_len == max_len


@pytest.mark.parametrize("switch", SWITCHES)
def test_the_route_switches_keep_their_meaning(ca, monkeypatch, switch):
    """read per call, each in a fresh context: every read in the full layout from the start; the full wave kernel instead of the
    light walk; an ASCII window of 512 bytes (most arrays go to the last-resort launch); rows of 8 entries (every edit distance of
    the wave form goes there)"""
    monkeypatch.setenv(switch, {"CRASS_SEQ_WINDOW": "512", "CRASS_ROW_CAP": "8"}.get(switch, "1"))
    gpu = ca.search_pipeline(seqs_up_to())
    assert_same_pipeline(gpu, reference())


def test_a_group_of_two_contexts(ca):
    gpu = ca.search_pipeline_group(seqs_up_to(), [0, 0], local_copies=True)
    gpu.counters = gpu.counters[0]
    assert_same_pipeline(gpu, reference())


def test_text_round_trip_of_the_found_records(ca):
    """fetch_text of every record's read, forward and reverse-complemented, and the records' RH_Seq, against the input"""
    from tests.test_gpu_fetch_text import revcomp
    seqs, ref = seqs_up_to(), reference()
    with ca.SearchEngine() as eng:
        eng.load_text(seqs)
        cand = eng.seed_scan()
        eng.merge()
        rec = eng.recruit()
        assert cand.read_idx.tolist() == ref.rec_read[:ref.n_pass1].tolist() and rec.read_idx.tolist() == ref.rec_read[ref.n_pass1:].tolist()
        idx = np.concatenate([cand.read_idx, rec.read_idx]).astype(np.uint64)
        low = np.concatenate([cand.low_lexi, rec.low_lexi]).astype(np.uint8)
        for what, flags, want in (("forward", None, [seqs[int(i)] for i in idx]),
                                  ("reversed", np.ones(len(idx), np.uint8), [revcomp(seqs[int(i)]) for i in idx]),
                                  ("as the records hold them", (1 - low).astype(np.uint8),
                                   [seqs[int(i)] if l else revcomp(seqs[int(i)]) for i, l in zip(idx, low)])):
            t = eng.fetch_text(idx, flags)
            assert t.n == len(idx) and t.off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist(), what
            assert t.chars.tobytes() == b"".join(want), what
        for p, (ri, lw) in ((1, (cand.read_idx, cand.low_lexi)), (2, (rec.read_idx, rec.low_lexi))):
            t = eng.fetch_record_text(p)
            assert t.chars.tobytes() == b"".join(seqs[int(i)] if l else revcomp(seqs[int(i)]) for i, l in zip(ri, lw)), p


def test_consensus_on_the_set(ca):
    from tests.test_gpu_consensus import assert_same_consensus
    seqs = seqs_up_to()
    search = ca.search_pipeline(seqs)
    assert_same_pipeline(search, reference())
    gpu = ca.consensus(seqs, search)
    ref = orc.consensus(seqs, reference())
    assert_same_consensus(gpu, ref)
    assert sorted(ref.true_drs) == sorted([S.DR_A, S.revcomp(S.DR_B)])


def test_options_whose_bounded_layout_passes_a_cu_are_still_refused(ca):
    """rows for a 14 000-base spacer (-S 14000) on top of a 60 000-base read's copy, list, words and hints: beyond 160 KB"""
    assert S.full_layout_bytes(60000, row_len=14000) > S.LDS_BYTES >= S.full_layout_bytes(60000, row_len=12000)
    with ca.SearchEngine(ca.default_params(highSpacerSize=14000)) as eng:
        eng.load_reads(ca.PackedReads(seqs_up_to()))
        with pytest.raises(ca.CrassError) as e:
            eng.seed_scan()
        assert e.value.status == 2


@pytest.mark.parametrize("reader", ["index", "device"])
def test_the_command_line_on_a_file_with_such_reads(cli, tmp_path, reader):
    """crass-hip end to end (search, consensus, graphs, output files) on a FASTQ file of the set, through the indexed reader and
    through the device ingest; the search's hand-off against the oracle"""
    from tests.test_gpu_adapter import parse_handoff, RC
    reads = S.get()
    path = tmp_path / "long.fq"
    path.write_bytes(b"".join(b"@%s c%d\n%s\n+\n%s\n" % (r.name.encode(), i, r.seq, bytes(70 + (i + k) % 40 for k in range(r.L)))
                              for i, r in enumerate(reads)))
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, CRASS_INGEST=reader, CRASS_TIMING="1")
    r = subprocess.run([cli, "-g", "-o", str(out), "--timestamp", STAMP, "--dump-handoff", str(path)], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    if reader == "device":
        assert "device ingest" in r.stderr.decode()
    ref = reference()
    h = parse_handoff(str(out / "crass_hip_handoff.tsv"))
    assert h["meta"]["max_read_length"] == S.MAX_READ_LEN
    assert [h["tokens"][t] for t in sorted(h["tokens"])] == ref.tokens
    assert [h["groups"][g] for g in sorted(h["groups"])] == ref.groups
    assert sorted(h["patterns"]) == sorted(ref.patterns)
    want = {}
    for k in range(ref.n_pass1 + ref.n_pass2):
        rd = reads[int(ref.rec_read[k])]
        low = int(ref.rec_lowlexi[k])
        want.setdefault(int(ref.rec_token[k]), []).append((rd.name.encode(), low, ref.ss(k), rd.seq if low else rd.seq.translate(RC)[::-1]))
    got = {t: [(x["header"], x["low"], x["ss"], x["seq"]) for x in v] for t, v in h["reads"].items()}
    assert got == want
    assert "2 true direct repeats" in r.stdout.decode()
