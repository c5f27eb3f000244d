"""crass_fastx_files_shards_host_class — the cut rule of csrc/fastx_scan.h for a FASTQ class on the host, no GPU — against the
brute-force statement of tests/shard_wrapped_sets.py: under class 1 the record starts of a FASTQ file are the header lines of the
records the wrapped rule walks from line 0.  Every byte of the decoy file as the nominal cut on 2 to 4 ranks, the designed jobs,
class 0 equal to crass_fastx_files_shards_host, the verdict equal to crass_fastx_files_scan_host_class(.., 1, ..) whatever the
cuts, the argument checks, and the stand-alone sanitizer program."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import shard_sets, shard_wrapped_sets as S, wrapped_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = S.cases()
DECLINED = S.declined()


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def same(a, b):
    return (a.accepted, a.n_ranks, a.n_files, a.n_reads, a.max_len, a.formats, a.cuts, a.verdict) == \
           (b.accepted, b.n_ranks, b.n_files, b.n_reads, b.max_len, b.formats, b.cuts, b.verdict) and \
           np.array_equal(a.rank_read_base, b.rank_read_base) and np.array_equal(a.file_read_base, b.file_read_base)


def assert_rule(ca, files, n_ranks, nominal, what):
    sh = ca.fastx_files_shards_host(files, n_ranks, nominal, fastq_class=1)
    cuts, base = S.brute_shards(files, n_ranks, nominal)
    assert sh.accepted and sh.n_ranks == n_ranks and sh.n_files == len(files), what
    assert sh.cuts == cuts, (what, sh.cuts, cuts)
    assert sh.rank_read_base.tolist() == base, (what, sh.rank_read_base, base)
    return sh


def test_the_decoy_file_is_what_it_says():
    reason, _, rec_pos, reads = wrapped_sets.judge(S.DECOY)
    assert reason == 0 and rec_pos == S.DECOY_STARTS and len(S.DECOY) == 113
    assert S.DECOY[S.DECOY_AT:S.DECOY_AT + 4] == b"@dec"
    # the bytes from the decoy on parse on their own as a valid chain — of records that are not the file's
    reason, _, own, _ = wrapped_sets.judge(S.DECOY[S.DECOY_AT:])
    assert reason == 0 and own[:3] == [0, 17, 40] and S.DECOY_AT + 17 == 77
    for x in range(41, 61):
        assert S.brute_shards([S.DECOY], 2, [x])[0][1] == (0, 77)
    # the four-line rule would cut at the decoy's line or decline: the file is outside that class
    assert wrapped_sets.judge(S.second_small())[0] == 0 and 100 < len(S.second_small()) < 200


def test_every_byte_of_the_decoy_as_the_nominal_cut(ca):
    files = [S.DECOY]
    T = len(S.DECOY)
    seen = set()
    for x in range(T + 1):
        seen.add(assert_rule(ca, files, 2, [x], x).cuts[1])
        for y in (x, min(T, x + 7), T):
            assert_rule(ca, files, 3, [x, y], (x, y))
            assert_rule(ca, files, 4, [x, y, T], (x, y, T))
            assert_rule(ca, files, 4, [0, x, y], (0, x, y))
    assert seen == {(0, p) for p in S.DECOY_STARTS[:-1]} | {(1, 0)}
    for x in range(41, 61):
        assert ca.fastx_files_shards_host(files, 2, [x], fastq_class=1).cuts[1] == (0, 77)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_designed_jobs(ca, name):
    files, positions, _ = CASES[name]
    for n in (2, 3, 4):
        for nominal in S.nominal_lists(files, positions, n):
            assert_rule(ca, files, n, nominal, (name, n, nominal))
    T = shard_sets.text_bases(files)[-1]
    for x in range(0, T + 1, 1 if T < 600 else 211):
        assert_rule(ca, files, 2, [x], (name, x))
    for n in range(1, 8):
        assert_rule(ca, files, n, None, (name, n))


@pytest.mark.parametrize("name", sorted(shard_sets.cases()))
def test_class_0_is_the_four_line_call(ca, name):
    files, positions = shard_sets.cases()[name]
    for n in (2, 3, 4):
        for nominal in shard_sets.nominal_lists(files, positions, n):
            a, b = ca.fastx_files_shards_host(files, n, nominal, fastq_class=0), ca.fastx_files_shards_host(files, n, nominal)
            assert same(a, b) and a.accepted, (name, n, nominal)
            # ... and a four-line job has the same records under either class
            assert same(ca.fastx_files_shards_host(files, n, nominal, fastq_class=1), a), (name, n, nominal)


def test_class_0_declines_what_it_declined(ca):
    for name, (files, _) in sorted(shard_sets.declined().items()):
        a, b = ca.fastx_files_shards_host(files, 3, None, fastq_class=0), ca.fastx_files_shards_host(files, 3)
        assert not a.accepted and same(a, b), name
    a = ca.fastx_files_shards_host([S.DECOY], 2, None, fastq_class=0)
    assert not a.accepted and a.verdict == ca.fastx_files_scan_host([S.DECOY]).verdict


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_the_verdict_is_the_class_scan_s_whatever_the_cuts(ca, name):
    files, positions = DECLINED[name]
    want = ca.fastx_files_scan_host(files, fastq_class=1)
    assert not want.accepted
    if len(files) == 1 and name in wrapped_sets.declines(S.TILE):
        _, reason, pos = wrapped_sets.declines(S.TILE)[name]
        assert (want.decline_file, want.decline_reason, want.decline_pos) == (0, reason, pos), name
    T = sum(len(f) for f in files)
    lists = [(n, nominal) for n in (2, 3, 4) for nominal in S.nominal_lists(files, positions, n)] if T else []
    lists += [(2, [x]) for x in range(0, T + 1, 1 if T < 400 else 97)] + [(n, None) for n in range(1, 6)]
    for n, nominal in lists:
        try:
            sh = ca.fastx_files_shards_host(files, n, nominal, fastq_class=1)
        except ca.CrassError as e:                                    # (a cut beyond the text of the files in front of the decline)
            assert e.status == 1 and nominal is not None
            continue
        assert not sh.accepted and sh.verdict == want.verdict, (name, n, nominal, sh.verdict, want.verdict)
        assert len(sh.rank_read_base) == 0 and len(sh.cut_pos) == 0


def test_argument_checks(ca):
    for cls in (-1, 2, 7):
        with pytest.raises(ca.CrassError) as e:
            ca.fastx_files_shards_host([S.DECOY], 2, None, fastq_class=cls)
        assert e.value.status == 1
    for n in (0, 65):
        with pytest.raises(ca.CrassError) as e:
            ca.fastx_files_shards_host([S.DECOY], n, None, fastq_class=1)
        assert e.value.status == 1
    for nominal in ([len(S.DECOY) + 1], ):
        with pytest.raises(ca.CrassError) as e:
            ca.fastx_files_shards_host([S.DECOY], 2, nominal, fastq_class=1)
        assert e.value.status == 1
    with pytest.raises(ca.CrassError) as e:
        ca.fastx_files_shards_host([S.DECOY], 3, [50, 40], fastq_class=1)
    assert e.value.status == 1
    lib = ca.load()
    assert lib.crass_fastx_files_shards_host_class(None, None, 0, 2, None, 1, None) == 1


def test_the_sanitizer_program(tmp_path):
    """tools/sanitize/shards_class_main.cpp: the host rule of both classes over the designed sets under AddressSanitizer + UBSan, a
    stand-alone program on the CPU"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "shards_class_asan")
    src = [os.path.join(ROOT, p) for p in ("crass_amd/csrc/fastx_scan.cpp", "crass_amd/csrc/bgzf.cpp", "tools/sanitize/shards_class_main.cpp")]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include")] + src + ["-o", exe])
    sets = tmp_path / "sets"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools/sanitize/shards_class_dump.py"), str(sets)], cwd=ROOT)
    r = subprocess.run([exe] + sorted(str(p) for p in sets.iterdir()), capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok  : 0 failures", (r.stdout[-2000:], r.stderr[-3000:])
    assert sum(1 for ln in r.stdout.splitlines() if ln.startswith("ok   job")) >= len(CASES) + len(DECLINED)
    assert not any(w in r.stderr for w in ("runtime error", "AddressSanitizer", "LeakSanitizer")), r.stderr[-3000:]
