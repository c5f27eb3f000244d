"""The wrapped FASTQ rule on the host (crass_fastx_scan_host_class, crass_fastx_files_scan_host_class; no GPU): every designed
input of tests/wrapped_sets.py against crass_read_fastx, every designed decline against its stated (position, reason), the
four-line class inside the wrapped one with the identical layout, seeded sweeps drawn from the class's grammar and their
one-byte mutations, the ABI's new symbols, and the rule's stand-alone program under AddressSanitizer + UBSan.  Every
comparison is exact equality."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import fastx_sets, wrapped_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 4096                                                 # the device scan's tile
NEW_SYMBOLS = ["crass_fastx_scan_host_class", "crass_fastx_files_scan_host_class", "crass_hip_set_fastq_class", "crass_hip_last_scan_classes"]


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


DESIGNED = wrapped_sets.designed(T)
DECLINES = wrapped_sets.declines(T)
REGULAR = fastx_sets.regular()
EDGE = fastx_sets.tile_edge(T)
IRREGULAR = fastx_sets.irregular(T)


def reader(ca, tmp_path, data):
    p = tmp_path / "in.fq"
    p.write_bytes(data)
    return ca.FastxFile(str(p))


def check_against_reader(ca, tmp_path, data, what, lay=None):
    """an accepted layout against crass_read_fastx on the same bytes: reads, seq_off, max_len, header ids"""
    if lay is None:
        lay = ca.fastx_scan_host(data, fastq_class=1)
    assert lay.accepted and lay.decline_pos == 0, (what, lay.decline_reason, lay.decline_pos)
    f = reader(ca, tmp_path, data)
    assert lay.format == data[:1]
    assert lay.n_reads == f.n_reads and lay.max_len == f.max_len, (what, lay.n_reads, f.n_reads, lay.max_len, f.max_len)
    assert lay.seq_off.dtype == np.uint64 and np.array_equal(lay.seq_off, f.seq_off), what
    assert len(lay.rec_pos) == lay.n_reads + 1 and int(lay.rec_pos[-1]) == len(data), what
    if data[:1] == b"@":
        reason, _, rec_pos, reads = wrapped_sets.judge(data)
        assert reason == 0 and rec_pos == lay.rec_pos.tolist(), what
        assert b"".join(reads) == f.seq.tobytes() and [len(r) for r in reads] == np.diff(f.seq_off.astype(np.int64)).tolist(), what
    hid = ca.fastx_header_ids(data, lay.rec_pos)
    assert np.array_equal(hid, f.header_id), what
    return lay, f


def same_layout(a, b):
    return (a.accepted, a.n_reads, a.format, a.max_len, a.decline_reason, a.decline_pos) == (b.accepted, b.n_reads, b.format, b.max_len, b.decline_reason, b.decline_pos) and \
        np.array_equal(a.rec_pos, b.rec_pos) and np.array_equal(a.seq_off, b.seq_off)


def test_new_symbols_are_exported_and_declared(ca):
    lib = ca.load()
    header = open(os.path.join(ROOT, "include", "crass_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", ca.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", nm))
    for name in NEW_SYMBOLS:
        assert name in ca.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported, name
        getattr(lib, name)
    assert "#define CRASS_FX_FQ_EMPTY_SEQ 12" in header and header.count("kseq.cpp:171-226") >= 6
    assert lib.crass_hip_abi_version() == 3 and "#define CRASS_HIP_ABI_VERSION 3" in header


def test_the_designed_inputs_are_what_they_say():
    d = DESIGNED
    for w in (1, 7, 60):
        lines = d["wrap%d" % w].split(b"\n")
        assert max(len(ln) for ln in lines if ln[:1] not in (b"@", b"+")) == w
    for L in (T - 1, T, T + 1):
        assert sum(1 for ln in d["line_of_%d" % L].split(b"\n") if len(ln) == L) == 4
    assert wrapped_sets.judge(d["one_base"])[3] == [b"A"]
    q = [ln[:1] for ln in d["quality_starts_with_at_and_plus"].split(b"\n")]
    assert q.count(b"+") > 8 and q.count(b"@") > 8
    for what in ("hdr", "plus", "qual", "qual2"):
        for name, at in (("%s_first_byte_of_tile" % what, T), ("%s_last_byte_of_tile" % what, 2 * T - 1)):
            assert d[name][at - 1:at] == b"\n" and d[name][at:at + 1] == (b"+" if what == "plus" else b"@"), name
    long_lines = [ln for ln in d["read_9000_wrap60"].split(b"\n") if len(ln) == 60]
    assert len(long_lines) == 300 and len(d["read_9000_wrap60"]) > 4 * T
    for n in wrapped_sets.COUNTS:
        assert len(wrapped_sets.judge(d["records_%d" % n])[3]) == n
    assert len(d["records_70001"]) < 3 << 20
    for name, data in d.items():
        assert wrapped_sets.judge(data)[0] == 0, name
        assert fastx_sets.in_regular_class(data) == (name in wrapped_sets.FOUR_LINE), name
    # read as headers, the quality lines of this file would offend
    data = d["quality_lines_look_like_headers"]
    at = data.index(b"@IIII>")
    assert wrapped_sets.judge(data[at:])[0] != 0


@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_inputs_match_the_reader(ca, tmp_path, name):
    check_against_reader(ca, tmp_path, DESIGNED[name], name)


@pytest.mark.parametrize("name", sorted(wrapped_sets.FOUR_LINE))
def test_four_line_designed_inputs_have_the_four_line_layout(ca, name):
    assert same_layout(ca.fastx_scan_host(DESIGNED[name], fastq_class=1), ca.fastx_scan_host(DESIGNED[name]))


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_designed_declines_get_their_verdict(ca, name):
    data, reason, pos = DECLINES[name]
    assert wrapped_sets.judge(data)[:2] == (reason, pos), (name, wrapped_sets.judge(data)[:2])
    lay = ca.fastx_scan_host(data, fastq_class=1)
    assert not lay.accepted and (lay.decline_reason, lay.decline_pos) == (reason, pos), (name, lay.decline_reason, lay.decline_pos, reason, pos)
    assert lay.n_reads == 0 and len(lay.rec_pos) == 0 and len(lay.seq_off) == 0


def test_every_wrapped_decline_reason_is_covered():
    assert {r for _, r, _ in DECLINES.values()} == {1, 2, 3, 4, 5, 7, 8, 9, 12}


@pytest.mark.parametrize("name", sorted(REGULAR) + sorted(EDGE))
def test_regular_inputs_have_the_same_layout_under_both_classes(ca, name):
    data = REGULAR.get(name, EDGE.get(name))
    a, b = ca.fastx_scan_host(data, fastq_class=1), ca.fastx_scan_host(data)
    assert b.accepted and same_layout(a, b), (name, a.decline_reason, a.decline_pos)


@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_irregular_inputs_are_declined_or_match_the_reader(ca, tmp_path, name):
    data = IRREGULAR[name][0]
    lay = ca.fastx_scan_host(data, fastq_class=1)
    assert (lay.decline_reason, lay.decline_pos) == wrapped_sets.judge(data)[:2] or data[:1] != b"@", name
    if data[:1] != b"@":
        assert same_layout(lay, ca.fastx_scan_host(data)), name
    if lay.accepted:
        check_against_reader(ca, tmp_path, data, name, lay)


def test_some_irregular_inputs_are_accepted_now(ca):
    accepted = {name for name, (data, _, _) in IRREGULAR.items() if ca.fastx_scan_host(data, fastq_class=1).accepted}
    assert {"fq_multi_line_first", "fq_multi_line_third_tile", "fq_multi_line_last", "fq_trailing_blank_line"} <= accepted


def test_class_zero_is_the_four_line_scan(ca):
    for name, data in list(DESIGNED.items()) + [(k, v[0]) for k, v in DECLINES.items()]:
        if len(data) < 1 << 16:
            lib = ca.load()
            v = ca._abi.FastxLayoutC()
            a = np.frombuffer(data, np.uint8)
            st = lib.crass_fastx_scan_host_class(a.ctypes.data if len(a) else None, len(a), 0, v)
            got = ca.engine.FastxLayout(v)
            lib.crass_fastx_layout_free(v)
            assert st in (0, 2) and same_layout(got, ca.fastx_scan_host(data)), name


def test_files_as_one_set(ca):
    files = [DESIGNED["four_line"], DESIGNED["wrap7"], REGULAR["wrap60"], DESIGNED["void_lines"]]
    lay = ca.fastx_files_scan_host(files, fastq_class=1)
    assert lay.accepted and lay.n_reads == sum(ca.fastx_scan_host(f, fastq_class=1).n_reads for f in files)
    at = 0
    for k, f in enumerate(files):
        one = ca.fastx_scan_host(f, fastq_class=1)
        r0, r1 = int(lay.file_read_base[k]), int(lay.file_read_base[k + 1])
        assert r1 - r0 == one.n_reads and np.array_equal(lay.rec_pos[r0:r1], one.rec_pos[:-1] + np.uint64(at)), k
        at += len(f) + 1
    with pytest.raises(Exception):
        ca.fastx_files_scan_host(files[:2] + [DECLINES["empty_then_at_first"][0]], fastq_class=2)
    bad = ca.fastx_files_scan_host(files[:2] + [DECLINES["empty_then_at_first"][0]], fastq_class=1)
    assert not bad.accepted and (bad.decline_file, bad.decline_reason, bad.decline_pos) == (2, 12, DECLINES["empty_then_at_first"][2])
    four = ca.fastx_files_scan_host(files, fastq_class=0)
    assert not four.accepted and four.decline_file == 1


def test_argument_errors(ca):
    lib = ca.load()
    v = ca._abi.FastxLayoutC()
    a = np.frombuffer(b"@a\nA\n+\nI\n", np.uint8)
    assert lib.crass_fastx_scan_host_class(a.ctypes.data, len(a), 2, v) == 1
    assert lib.crass_fastx_scan_host_class(a.ctypes.data, len(a), -1, v) == 1
    assert lib.crass_fastx_scan_host_class(None, 5, 1, v) == 1
    assert lib.crass_fastx_scan_host_class(a.ctypes.data, len(a), 1, None) == 1


def test_generated_sweep_is_accepted_and_matches_the_reader(ca, tmp_path):
    """2 000 files drawn from the class's grammar (the generator asserts membership by the Python rule): all accepted, all equal
    to crass_read_fastx — a scan that declines its way to a pass fails here"""
    rng = random.Random(20261021)
    for k in range(2000):
        data = wrapped_sets.generate(rng)
        check_against_reader(ca, tmp_path, data, (k, data))


def test_mutated_sweep_agrees_with_the_reader_wherever_it_accepts(ca, tmp_path):
    """2 000 one-byte mutations of generated files: the verdict is the Python rule's, and an accepted one equals crass_read_fastx"""
    rng = random.Random(20261022)
    accepted = 0
    for k in range(2000):
        data = wrapped_sets.mutate(rng, wrapped_sets.generate(rng))
        lay = ca.fastx_scan_host(data, fastq_class=1)
        if data[:1] == b"@":
            assert (lay.decline_reason, lay.decline_pos) == wrapped_sets.judge(data)[:2], (k, data)
        if lay.accepted:
            accepted += 1
            check_against_reader(ca, tmp_path, data, (k, data), lay)
        else:
            assert 1 <= lay.decline_reason <= 12 and lay.decline_pos <= len(data) and lay.n_reads == 0, (k, data)
    print("mutations accepted: %d of 2000" % accepted)


def test_sanitizer_program_builds_and_runs_clean(tmp_path):
    """tools/sanitize/wrapped_scan_main.cpp: the host rule over its built-in inputs and all their prefixes under
    -fsanitize=address,undefined, a stand-alone program on the CPU, the sanitizer runtimes linked statically and nothing preloaded"""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path / "wrapped_scan_asan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "crass_amd", "csrc", "fastx_scan.cpp"), os.path.join(ROOT, "crass_amd", "csrc", "bgzf.cpp"),
                    os.path.join(ROOT, "tools", "sanitize", "wrapped_scan_main.cpp"), "-o", exe, "-lz"], check=True, capture_output=True, text=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "DIFF" not in r.stdout and r.stdout.strip().splitlines()[-1].startswith("passed")
    assert not re.search(r"AddressSanitizer|runtime error|LeakSanitizer", r.stderr), r.stderr[-2000:]
