"""crass_fastx_files_scan_host — several input files as one read set, on the host — against crass_index_fastx_files on the same
files written to disk: read count, longest read, every read's text, header ids across the files and the files' read bases; the
declined sets' verdicts (the first file in order wins); the header's declarations; the ABI version.  No GPU."""
import os
import re

import numpy as np
import pytest

import crass_amd as ca
from crass_amd import engine as E
from tests import files_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED = files_sets.accepted()
DECLINED = files_sets.declined()


@pytest.fixture(scope="module", autouse=True)
def lib():
    return ca.load()


def unpack(words, length, exc):
    if exc is not None:
        return exc
    return bytes(b"ACGT"[(int(words[i // 16]) >> (2 * (i % 16))) & 3] for i in range(length))


def joined(files, lay):
    """the arena as the layout describes it, and every read's text cut out of it by the scan's own rule"""
    texts = files_sets.text_of(files)
    arena = b"".join(t + b"\n" for t in texts)
    reads = []
    for r in range(lay.n_reads):
        rec = arena[int(lay.rec_pos[r]):int(lay.rec_pos[r + 1])]
        lines = rec.split(b"\n")
        body = lines[1:2] if rec[:1] == b"@" else lines[1:]
        reads.append(bytes(b for l in body for b in l if 33 <= b <= 126))
    return arena, reads


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_joined_layout_equals_the_indexed_reader(name, tmp_path):
    files = ACCEPTED[name]
    lay = E.fastx_files_scan_host(files)
    assert lay.accepted and lay.verdict == (-1, 0, 0, (0, 0, 0)), lay.verdict
    paths = []
    for k, f in enumerate(files):
        p = tmp_path / ("f%d%s" % (k, ".gz" if f[:2] == b"\x1f\x8b" else ".fx"))
        p.write_bytes(f)
        paths.append(str(p))
    ix = E.FastxIndex(paths)
    want = ix.layout()
    assert lay.n_files == len(files) and lay.n_reads == ix.n_reads and lay.max_len == ix.max_len
    arena, reads = joined(files, lay)
    texts = files_sets.text_of(files)
    # bases: file f's text lies at its byte base, a '\n' behind it; its reads start at its read base
    at = 0
    for f, t in enumerate(texts):
        assert int(lay.file_byte_base[f]) == at and lay.formats[f] == t[:1]
        at += len(t) + 1
    assert int(lay.file_byte_base[-1]) == at == len(arena) and int(lay.rec_pos[-1]) == at - 1
    per_file = [len(E.FastxIndex(p).layout()["lengths"]) for p in paths]
    assert lay.file_read_base.tolist() == np.concatenate([[0], np.cumsum(per_file)]).tolist()
    # every read's text and its place in the joined sequence text
    assert (np.diff(lay.seq_off.astype(np.int64)) == np.array(want["lengths"], np.int64)).all() and int(lay.seq_off[0]) == 0
    for r in range(lay.n_reads):
        assert reads[r] == unpack(want["words"][r], want["lengths"][r], want["exceptions"].get(r)), r
        assert arena[int(lay.rec_pos[r])] in b">@"
    # header ids over all files, from the arena: the '\n' behind a file ends the name of a last record without a line end
    assert E.fastx_header_ids(arena, lay.rec_pos).tolist() == want["header_id"]
    ix.close()


def test_one_file_equals_the_single_file_scan():
    (f,) = ACCEPTED["one_file"]
    lay, one = E.fastx_files_scan_host([f]), E.fastx_scan_host(f)
    assert lay.accepted and one.accepted
    assert (lay.n_reads, lay.max_len, lay.formats) == (one.n_reads, one.max_len, [one.format])
    assert lay.rec_pos.tolist() == one.rec_pos.tolist() and lay.seq_off.tolist() == one.seq_off.tolist()
    assert lay.file_read_base.tolist() == [0, one.n_reads] and lay.file_byte_base.tolist() == [0, len(f) + 1]


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_sets_name_the_first_offending_file(name):
    files, want = DECLINED[name]
    lay = E.fastx_files_scan_host(files)
    assert not lay.accepted and lay.n_files == len(files)
    assert files_sets.verdict_of(lay) == want
    assert len(lay.rec_pos) == 0 and len(lay.seq_off) == 0 and lay.n_reads == 0


def test_a_single_file_decline_is_the_single_file_scan_s():
    bad = b"@r\nACGT\n+\nII\n"                              # a quality line shorter than its sequence line
    lay, one = E.fastx_files_scan_host([ACCEPTED["one_file"][0], bad]), E.fastx_scan_host(bad)
    assert (lay.decline_file, lay.decline_reason, lay.decline_pos) == (1, one.decline_reason, one.decline_pos) and one.decline_reason == 8


def test_invalid_arguments():
    lib = ca.load()
    from crass_amd import _abi
    import ctypes as C
    v = _abi.FastxFilesLayoutC()
    assert lib.crass_fastx_files_scan_host(None, None, 0, C.byref(v)) == 1
    assert lib.crass_fastx_files_scan_host(None, None, 1, None) == 1


def test_header_declares_the_new_functions_and_the_abi_version_stays():
    h = open(os.path.join(ROOT, "include", "crass_hip.h")).read()
    for fn in ("crass_hip_load_fastx_files", "crass_hip_resident_fastx", "crass_fastx_files_scan_host", "crass_fastx_files_layout_free",
               "crass_hip_fetch_quality_device", "crass_hip_fetch_quality_device_to"):
        assert re.search(r"\bint\s+%s\(|\bvoid\s+%s\(" % (fn, fn), h), fn
        assert hasattr(ca.load(), fn), fn
    assert "crass_index_fastx_files + crass_fastx_index_reads + crass_hip_load_reads" in h and "libcrispr.cpp:96-131" in h
    assert ca.load().crass_hip_abi_version() == 3
