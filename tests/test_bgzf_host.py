"""BGZF on the host (crass_bgzf_index_host / crass_bgzf_inflate_host, csrc/bgzf.cpp + csrc/inflate_core.h — the decoder the kernel
runs): the index against a Python restatement of the header walk, the text and the verdicts against zlib, the new walk tied to the
existing readers, and the sanitizer run of the same code as a stand-alone program.  No GPU.  Every comparison is exact equality."""
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import bgzf_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGULAR = bgzf_sets.regular()
DAMAGED = bgzf_sets.damaged()
NOT_BGZF = bgzf_sets.not_bgzf()
NEW_SYMBOLS = ["crass_bgzf_index_host", "crass_bgzf_index_free", "crass_bgzf_inflate_host", "crass_hip_inflate_bgzf_device",
               "crass_hip_load_fastx_bgzf", "crass_hip_last_inflate_ms"]


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def test_the_new_calls_are_declared_bound_and_cite_what_they_replace(ca):
    hdr = open(os.path.join(ROOT, "include", "crass_hip.h")).read()
    lib = ca.load()
    for name in NEW_SYMBOLS:
        assert name in ca.SYMBOLS and hasattr(lib, name), name
        assert name + "(" in hdr, name
    assert hdr.count("SeqUtils.cpp:100-126") >= 4 and "getFileHandle / gzopen" in hdr
    assert lib.crass_hip_abi_version() == 3
    for name in ("bgzf_index", "bgzf_inflate_host", "BgzfDeclined", "BgzfIndex"):
        assert hasattr(ca, name), name
    assert hasattr(ca.SearchEngine, "inflate_bgzf_device") and hasattr(ca.SearchEngine, "load_fastx_bgzf")


@pytest.mark.parametrize("name", sorted(REGULAR) + ["damaged " + k for k in sorted(DAMAGED)])
def test_index_is_the_header_walk(ca, name):
    data = DAMAGED[name[8:]][0] if name.startswith("damaged ") else REGULAR[name]
    (ioff, ooff, doff), _, _ = bgzf_sets.walk(data)
    ix = ca.bgzf_index(data)
    assert ix.n_members == len(doff) and ix.n_text == ooff[-1]
    assert ix.in_off.tolist() == ioff and ix.out_off.tolist() == ooff and ix.data_off.tolist() == doff


@pytest.mark.parametrize("name", sorted(NOT_BGZF))
def test_what_is_not_bgzf_is_declined_at_the_member_that_does_not_parse(ca, name):
    data, member, pos = NOT_BGZF[name]
    assert bgzf_sets.walk(data) == (None, pos, member)
    for call in (ca.bgzf_index, ca.bgzf_inflate_host):
        with pytest.raises(ca.BgzfDeclined) as e:
            call(data)
        assert e.value.status == 2 and e.value.verdict == (bgzf_sets.NOT_BGZF, member, pos)


@pytest.mark.parametrize("name", sorted(REGULAR))
def test_text_is_zlibs(ca, name):
    data = REGULAR[name]
    members = bgzf_sets.zlib_members(data)
    assert all(ok for _, ok in members)
    assert ca.bgzf_inflate_host(data).tobytes() == b"".join(t for t, _ in members)


def test_hand_made_streams_hold_what_they_are_named_for(ca):
    """the streams zlib does not write, member by member, against the text their tokens spell"""
    for name, (m, text) in bgzf_sets.hand_made_members().items():
        assert ca.bgzf_inflate_host(m).tobytes() == text, name
        assert zlib.decompress(m, 31) == text, name


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damaged_files_get_their_member_and_reason(ca, name):
    data, member, reason = DAMAGED[name]
    ix = ca.bgzf_index(data)
    members = bgzf_sets.zlib_members(data)
    assert [i for i, (_, ok) in enumerate(members) if not ok][0] == member        # zlib's first complaint is about that member
    with pytest.raises(ca.BgzfDeclined) as e:
        ca.bgzf_inflate_host(data)
    assert e.value.status == 2 and e.value.verdict == (reason, member, int(ix.in_off[member]))


def test_single_bit_flips_never_give_another_text(ca):
    declined = accepted = 0
    for data, hit in bgzf_sets.bit_flips():
        members = bgzf_sets.zlib_members(data)
        bad = [i for i, (_, ok) in enumerate(members) if not ok]
        assert bad in ([], [hit])
        try:
            got = ca.bgzf_inflate_host(data).tobytes()
        except ca.BgzfDeclined as e:
            assert 1 <= e.reason <= 9 and e.member == hit
            assert bad == [hit]                           # no decline of a member that zlib and its trailer accept
            declined += 1
            continue
        assert not bad and got == b"".join(t for t, _ in members)
        accepted += 1
    assert declined + accepted == 200 and declined >= 150


def test_argument_checks(ca):
    lib = ca.load()
    data = np.frombuffer(REGULAR["members_65"], np.uint8)
    ix = ca.bgzf_index(data)
    out = np.full(ix.n_text + 64, 0xA7, np.uint8)
    ptr, n = data.ctypes.data, len(data)
    assert lib.crass_bgzf_inflate_host(ptr, n, ix._c(), out.ctypes.data + 32, ix.n_text - 1, None) == 1      # out_cap < out_off[n]
    assert lib.crass_bgzf_inflate_host(ptr, n - 1, ix._c(), out.ctypes.data + 32, ix.n_text, None) == 1      # beyond n_bytes
    assert lib.crass_bgzf_inflate_host(None, n, ix._c(), out.ctypes.data + 32, ix.n_text, None) == 1
    assert lib.crass_bgzf_inflate_host(ptr, n, ix._c(), None, ix.n_text, None) == 1
    assert lib.crass_bgzf_inflate_host(ptr, n, None, out.ctypes.data + 32, ix.n_text, None) == 1
    off = ix.out_off.copy(); off[2] = off[3] + 1
    assert lib.crass_bgzf_inflate_host(ptr, n, ca.BgzfIndex(ix.in_off, off, ix.data_off)._c(), out.ctypes.data + 32, ix.n_text, None) == 1
    far = ix.data_off.copy(); far[5] = ix.in_off[6]
    assert lib.crass_bgzf_inflate_host(ptr, n, ca.BgzfIndex(ix.in_off, ix.out_off, far)._c(), out.ctypes.data + 32, ix.n_text, None) == 1
    assert np.all(out == 0xA7)                            # nothing was written
    assert lib.crass_bgzf_inflate_host(ptr, n, ix._c(), out.ctypes.data + 32, ix.n_text, None) == 0          # v may be NULL
    assert np.all(out[:32] == 0xA7) and np.all(out[32 + ix.n_text:] == 0xA7)
    assert lib.crass_bgzf_index_host(None, 5, None) == 1


@pytest.mark.parametrize("name", bgzf_sets.fastx_regular())
def test_the_existing_reader_sees_the_same_reads(ca, tmp_path, name):
    """crass_index_fastx on the file (bgzf_walk + the side-by-side inflate where the file has more than 64 members, the serial
    readers below that) against the record scan of the new functions' text"""
    data = REGULAR[name]
    text = ca.bgzf_inflate_host(data)
    lay = ca.fastx_scan_host(text)
    assert lay.accepted
    p = tmp_path / "in.fq.gz"
    p.write_bytes(data)
    ix = ca.FastxIndex(str(p))
    try:
        assert ix.n_reads == lay.n_reads and ix.max_len == lay.max_len
        raw = text.tobytes()
        seqs = []
        for r in range(lay.n_reads):
            lines = raw[int(lay.rec_pos[r]):int(lay.rec_pos[r + 1])].split(b"\n")
            body = lines[1:2] if lay.format == b"@" else lines[1:]
            seqs.append(bytes(c for c in b"".join(body) if 33 <= c <= 126))
        assert [rec[2] for rec in ix.fetch(list(range(lay.n_reads)))] == seqs
    finally:
        ix.close()


def test_sanitizer_program_is_clean(tmp_path):
    """tools/sanitize/bgzf_main.cpp: the host code and a main of its own under AddressSanitizer + UBSan, as a stand-alone program
    over every set (exact-size heap buffers around input and output).  The sanitizer runtimes are linked statically, so the
    program does not care what else the environment loads in front of it; the environment is passed on as it is."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "bgzf_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "crass_amd", "csrc", "bgzf.cpp"), os.path.join(ROOT, "tools", "sanitize", "bgzf_main.cpp"), "-o", exe])
    d = tmp_path / "files"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "sanitize", "bgzf_dump.py"), str(d)])
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + sorted(str(p) for p in d.iterdir()), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "0 DIFF" in r.stdout.splitlines()[-1] and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
