"""The comment kseq hands on from record to record, on the host (crass_fastx_comments_of; no GPU): against the has_comment /
comment arrays of crass_read_fastx — the reader that is pinned against the compiled kseq.cpp in test_abi.py — file by file on
every designed job of tests/comment_sets.py, for all records in order and for lists in any order with repeats, with both index
bases; the status-code table (the capacity one byte short, exact and one byte long with the bytes behind it left alone; indices
out of range; NULL arrays; a file_read_base that does not fit; n == 0); and tools/sanitize/comments_of_main.cpp as a
stand-alone program under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import comment_sets as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = cs.jobs()
FILL = 0xA5
INVALID_ARG, OVERFLOW = 1, 8


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def reference(ca, tmp_path_factory):
    """per job: (arena bytes, layout, has [n], list of comments) — the last two from crass_read_fastx, file by file"""
    d = tmp_path_factory.mktemp("comment_sets")
    out = {}
    for name, files in JOBS.items():
        lay = ca.fastx_files_scan_host(files)
        assert lay.accepted, (name, lay.verdict)
        has, com = [], []
        for f, text in enumerate(files):
            assert ca.fastx_scan_host(text).accepted, (name, f)
            p = d / ("%s_%d.%s" % (name, f, "fq" if text[:1] == b"@" else "fa"))
            p.write_bytes(text)
            fx = ca.FastxFile(p)
            assert fx.n_reads == int(lay.file_read_base[f + 1] - lay.file_read_base[f]), (name, f)
            for i in range(fx.n_reads):
                has.append(int(fx.has_comment[i]))
                com.append(fx._field(fx.comment, fx.comment_off, i) if fx.has_comment[i] else b"")
        out[name] = (cs.arena(files), lay, np.asarray(has, np.uint8), com)
    return out


def test_the_model_says_what_the_reader_says(reference):
    """comment_sets.model, which the other tests use to describe a set, agrees with crass_read_fastx on every job; the mixed
    jobs really hand comments on that are not on the record's own line"""
    for name, files in JOBS.items():
        _, _, has, com = reference[name]
        m = cs.model(files)
        assert [x[0] for x in m] == has.tolist() and [x[1] for x in m] == com, name
    assert sum(1 for h, _, own in cs.model(JOBS["every_third"]) if h and not own) == 20
    assert sum(1 for h, _, own in cs.model(JOBS["sparse"]) if h and not own) == 12300 - 4096
    assert sum(1 for h, _, own in cs.model(JOBS["two_files"]) if h and not own) == 0


@pytest.mark.parametrize("name", sorted(JOBS))
def test_comments_of_equals_the_reader(ca, reference, name):
    data, lay, has, com = reference[name]
    n = lay.n_reads
    for idx in (list(range(n)), cs.picks(name, n)):
        want_c, want_o = cs.concat([com[r] for r in idx])
        for base in (0, 7):
            c, o, h = ca.comments_of(data, lay.rec_pos, np.asarray(idx, np.uint64) + np.uint64(base), lay.file_read_base, idx_base=base)
            assert np.array_equal(o, want_o) and np.array_equal(c, want_c) and np.array_equal(h, has[idx]), (name, base)
    if lay.n_files == 1:                                 # NULL file_read_base means one file
        c, o, h = ca.comments_of(data, lay.rec_pos, list(range(n)))
        want_c, want_o = cs.concat(com)
        assert np.array_equal(o, want_o) and np.array_equal(c, want_c) and np.array_equal(h, has), name


def test_sparse_queries_reach_the_carry_across_an_empty_tile(ca, reference):
    data, lay, has, com = reference["sparse"]
    c, o, h = ca.comments_of(data, lay.rec_pos, cs.SPARSE_QUERIES, lay.file_read_base)
    assert h.tolist() == [1, 1, 1, 1, 1, 0, 0] and bytes(c) == b"only" * 5 and o.tolist() == [0, 4, 8, 12, 16, 20, 20, 20]


def test_nothing_carries_across_a_file_boundary(ca, reference):
    data, lay, has, com = reference["two_files"]
    assert has.tolist() == [1] * 10 + [0] * 10
    # ... but it would within one file: the same bytes as one file of 20 records
    c, o, h = ca.comments_of(data, lay.rec_pos, list(range(20)))
    assert h.tolist() == [1] * 20 and bytes(c[int(o[10]):]) == com[9] * 10


def raw(ca, data, lay, idx, base, cap, guard=8, frb=True):
    """the C call itself into a buffer of cap bytes with a guard of FILL bytes behind it: (status, buffer, offsets, has)"""
    a = np.frombuffer(data, np.uint8)
    ix = np.asarray(idx, np.uint64) + np.uint64(base)
    out = np.full(cap + guard, FILL, np.uint8)
    off = np.full(len(ix) + 1, 2 ** 64 - 1, np.uint64)
    has = np.full(max(len(ix), 1), 9, np.uint8)
    fb = np.ascontiguousarray(lay.file_read_base, np.uint64)
    st = ca.load().crass_fastx_comments_of(a.ctypes.data, len(a), lay.rec_pos.ctypes.data, lay.n_reads, fb.ctypes.data if frb else None, len(fb) - 1 if frb else 0,
                                           ix.ctypes.data if len(ix) else None, len(ix), base, out.ctypes.data, cap, off.ctypes.data, has.ctypes.data)
    return st, out, off, has[:len(ix)]


@pytest.mark.parametrize("name", ["every_third", "empty_own", "long_comment", "three_files", "open_end_comment"])
def test_status_codes(ca, reference, name):
    data, lay, has, com = reference[name]
    idx = cs.picks(name, lay.n_reads)
    want_c, want_o = cs.concat([com[r] for r in idx])
    total = int(want_o[-1])
    for base in (0, 7):
        for cap in (total - 1, total, total + 1, 0):
            st, out, off, h = raw(ca, data, lay, idx, base, cap)
            assert st == (OVERFLOW if cap < total else 0), (name, cap)
            assert np.array_equal(off, want_o) and np.array_equal(h, has[idx])      # complete either way
            m = min(cap, total)
            assert np.array_equal(out[:m], want_c[:m]) and np.all(out[m:] == FILL), (name, cap)
        # n == 0
        st, out, off, h = raw(ca, data, lay, [], base, 0)
        assert st == 0 and off.tolist() == [0] and np.all(out == FILL)
        # an index out of range, below and above: nothing is written
        n = lay.n_reads
        for bad in ([0, n], [n + 5], [2 ** 63]):
            st, out, off, h = raw(ca, data, lay, bad, base, 64)
            assert st == INVALID_ARG and np.all(out == FILL) and np.all(off == 2 ** 64 - 1) and np.all(h == 9), (name, bad)
    a = np.frombuffer(data, np.uint8)
    ix = np.asarray([6], np.uint64)                      # below the base
    out = np.full(64, FILL, np.uint8)
    off = np.full(2, 5, np.uint64)
    st = ca.load().crass_fastx_comments_of(a.ctypes.data, len(a), lay.rec_pos.ctypes.data, lay.n_reads, None, 0, ix.ctypes.data, 1, 7, out.ctypes.data, 64,
                                           off.ctypes.data, None)
    assert st == INVALID_ARG and np.all(out == FILL) and off.tolist() == [5, 5]


def test_argument_errors(ca, reference):
    data, lay, has, com = reference["three_files"]
    lib = ca.load()
    a = np.frombuffer(data, np.uint8)
    rp, n = lay.rec_pos, lay.n_reads
    fb = np.ascontiguousarray(lay.file_read_base, np.uint64)
    ix = np.zeros(1, np.uint64)
    off = np.full(2, 5, np.uint64)
    call = lib.crass_fastx_comments_of
    assert call(a.ctypes.data, len(a), rp.ctypes.data, n, fb.ctypes.data, 3, None, 1, 0, None, 0, off.ctypes.data, None) == INVALID_ARG
    assert call(a.ctypes.data, len(a), rp.ctypes.data, n, fb.ctypes.data, 3, ix.ctypes.data, 1, 0, None, 0, None, None) == INVALID_ARG
    assert call(None, len(a), rp.ctypes.data, n, fb.ctypes.data, 3, ix.ctypes.data, 1, 0, None, 0, off.ctypes.data, None) == INVALID_ARG
    assert call(a.ctypes.data, len(a), None, n, fb.ctypes.data, 3, ix.ctypes.data, 1, 0, None, 0, off.ctypes.data, None) == INVALID_ARG
    assert call(a.ctypes.data, len(a), rp.ctypes.data, n, fb.ctypes.data, 3, ix.ctypes.data, 1, 0, None, 5, off.ctypes.data, None) == INVALID_ARG
    for bad in ([1, 100, 150, n], [0, 100, 150, n - 1], [0, 150, 100, n]):      # does not start at 0, does not end at n_reads, decreases
        b = np.asarray(bad, np.uint64)
        assert call(a.ctypes.data, len(a), rp.ctypes.data, n, b.ctypes.data, 3, ix.ctypes.data, 1, 0, None, 0, off.ctypes.data, None) == INVALID_ARG, bad
    assert call(a.ctypes.data, len(a), rp.ctypes.data, n, fb.ctypes.data, 0, ix.ctypes.data, 1, 0, None, 0, off.ctypes.data, None) == INVALID_ARG
    far = rp.copy()
    far[3] = len(a)                                      # a record position at the input's end
    assert call(a.ctypes.data, len(a), far.ctypes.data, n, fb.ctypes.data, 3, ix.ctypes.data, 1, 0, None, 0, off.ctypes.data, None) == INVALID_ARG
    assert off.tolist() == [5, 5]
    with pytest.raises(ca.CrassError) as err:
        ca.comments_of(data, rp, [n], fb)
    assert err.value.status == INVALID_ARG
    with pytest.raises(ca.CrassError) as err:
        ca.comments_of(data, rp, [2, 3], fb, cap_bytes=1)
    assert err.value.status == OVERFLOW and err.value.offsets.tolist() == [0, len(com[2]), len(com[2]) + len(com[3])] and err.value.has.tolist() == [1, 1]


def test_sanitizer_program_is_clean(tmp_path):
    """tools/sanitize/comments_of_main.cpp: the host function and a main of its own under AddressSanitizer + UBSan, as a
    stand-alone child process over designed jobs of its own (exact-size heap buffers around every array), the sanitizer runtimes
    linked statically and nothing preloaded."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "comments_of_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "crass_amd", "csrc", "fastx_scan.cpp"), os.path.join(ROOT, "crass_amd", "csrc", "bgzf.cpp"),
                           os.path.join(ROOT, "tools", "sanitize", "comments_of_main.cpp"), "-o", exe])
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) >= 20 and all(x.startswith("ok  ") for x in lines) and lines[-1] == "ok  : 0 failures", lines
    assert not any(w in r.stderr for w in ("runtime error", "AddressSanitizer", "LeakSanitizer")), r.stderr[-3000:]
