"""The record scan by lines on the host (crass_fastx_scan_host, crass_fastx_header_ids; no GPU): the ABI's new symbols, the scan
against crass_read_fastx on every regular input, the verdict on every irregular one, and a seeded sweep of small random files —
wherever the scan accepts it must agree with crass_read_fastx, and it must accept exactly the regular class.  Every comparison
is exact equality."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import fastx_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 4096                                                 # the device scan's tile (checked against the library where there is a GPU test)
NEW_SYMBOLS = ["crass_fastx_scan_host", "crass_fastx_layout_free", "crass_hip_load_fastx_bytes", "crass_hip_attach_device_fastx",
               "crass_hip_set_header_ids", "crass_fastx_header_ids", "crass_hip_fastx_tile_bytes", "crass_hip_last_scan_ms"]


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


REGULAR = fastx_sets.regular()
EDGE = fastx_sets.tile_edge(T)
IRREGULAR = fastx_sets.irregular(T)


def kseq(ca, tmp_path, data):
    p = tmp_path / "in.fx"
    p.write_bytes(data)
    return ca.FastxFile(str(p))


def check_against_kseq(ca, tmp_path, data, what):
    lay = ca.fastx_scan_host(data)
    assert lay.accepted and lay.decline_pos == 0, (what, lay.decline_reason, lay.decline_pos)
    f = kseq(ca, tmp_path, data)
    assert lay.format == data[:1]
    assert lay.n_reads == f.n_reads and lay.max_len == f.max_len, (what, lay.n_reads, f.n_reads, lay.max_len, f.max_len)
    assert lay.seq_off.dtype == np.uint64 and np.array_equal(lay.seq_off, f.seq_off), what
    assert len(lay.rec_pos) == lay.n_reads + 1 and int(lay.rec_pos[-1]) == len(data), what
    assert all(data[int(p):int(p) + 1] == data[:1] for p in lay.rec_pos[:-1]), what
    reads = fastx_sets.reads_by_rule(data, lay.rec_pos)
    assert b"".join(reads) == f.seq.tobytes() and [len(r) for r in reads] == np.diff(f.seq_off.astype(np.int64)).tolist(), what
    hid = ca.fastx_header_ids(data, lay.rec_pos)
    assert hid.dtype == np.uint64 and np.array_equal(hid, f.header_id), what
    return lay, f


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
    assert "crass_fastx_layout" in header
    assert lib.crass_hip_abi_version() == 3 and "#define CRASS_HIP_ABI_VERSION 3" in header
    assert lib.crass_hip_fastx_tile_bytes() == T


@pytest.mark.parametrize("name", sorted(REGULAR))
def test_regular_inputs_match_the_reader(ca, tmp_path, name):
    assert fastx_sets.in_regular_class(REGULAR[name]), name
    check_against_kseq(ca, tmp_path, REGULAR[name], name)


@pytest.mark.parametrize("name", sorted(EDGE))
def test_tile_edge_inputs_match_the_reader(ca, tmp_path, name):
    assert fastx_sets.in_regular_class(EDGE[name]), name
    check_against_kseq(ca, tmp_path, EDGE[name], name)


def test_tile_edge_inputs_are_where_they_should_be():
    e = EDGE
    assert e["hdr_first_byte_of_tile"][T:T + 5] == b">edge" and e["hdr_last_byte_of_tile"][T - 1:T + 4] == b">edge"
    assert e["nl_last_byte_of_tile"][T - 1:T] == b"\n" and e["hdr_nl_last_byte_of_tile"][2 * T - 1:2 * T] == b"\n"
    assert any(len(ln) == 2 * T + 4 and ln[:1] == b">" for ln in e["long_header"].split(b"\n"))
    assert any(len(ln) == 2 * T + 4 and ln[:1] != b">" for ln in e["long_seq_line"].split(b"\n"))
    assert b"\n" not in e["tile_without_newline"][T:2 * T]
    assert (len(e["exactly_T"]), len(e["T_minus_1"]), len(e["T_plus_1"]), len(e["T_plus_1_name_in_next_tile"])) == (T, T - 1, T + 1, T + 1)
    assert e["fq_hdr_first_byte_of_tile"][T:T + 5] == b"@edge" and e["fq_hdr_last_byte_of_tile"][T - 1:T + 4] == b"@edge"
    d = e["fq_four_tiles"]
    starts = [T - 10]
    for _ in range(3):
        starts.append(d.index(b"\n", starts[-1]) + 1)
    assert len({s // T for s in starts}) == 4
    for name, data in e.items():
        assert 0 < len(data) <= 5 * T + 200, name


def test_duplicate_names_give_the_first_read(ca, tmp_path):
    lay, f = check_against_kseq(ca, tmp_path, REGULAR["dup_names"], "dup_names")
    hid = ca.fastx_header_ids(REGULAR["dup_names"], lay.rec_pos)
    assert hid[:6].tolist() == [0, 1, 0, 3, 1, 0] and not f.unique_headers()


@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_irregular_inputs_are_declined(ca, name):
    data, reason, pos = IRREGULAR[name]
    assert not fastx_sets.in_regular_class(data), name
    lay = ca.fastx_scan_host(data)
    assert not lay.accepted and (lay.decline_reason, lay.decline_pos) == (reason, pos), (name, lay.decline_reason, lay.decline_pos, reason, pos)
    assert lay.n_reads == 0 and len(lay.rec_pos) == 0 and len(lay.seq_off) == 0
    lib = ca.load()
    v = ca._abi.FastxLayoutC()
    a = np.frombuffer(data, np.uint8)
    assert lib.crass_fastx_scan_host(a.ctypes.data if len(a) else None, len(a), v) == 2      # CRASS_ERR_UNSUPPORTED
    assert not v.rec_pos and not v.seq_off


def test_every_decline_reason_is_covered():
    assert {r for _, r, _ in IRREGULAR.values()} == set(range(1, 11))


def test_argument_errors(ca):
    lib = ca.load()
    v = ca._abi.FastxLayoutC()
    assert lib.crass_fastx_scan_host(None, 5, v) == 1
    assert lib.crass_fastx_scan_host(None, 0, None) == 1
    out = np.zeros(2, np.uint64)
    assert lib.crass_fastx_header_ids(None, 0, None, 2, out.ctypes.data) == 1
    assert lib.crass_fastx_header_ids(None, 0, None, 0, None) == 0
    lib.crass_fastx_layout_free(None)


def test_seeded_sweep_agrees_with_the_reader_wherever_it_accepts(ca, tmp_path):
    """2 400 draws of fastx_sets.random_input: the scan accepts exactly the regular class, agrees with crass_read_fastx on every
    accepted input, and accepts at least 80 % of the draws (a scan that declines its way to a pass fails here)"""
    rng = random.Random(20261018)
    n, accepted = 2400, 0
    for k in range(n):
        data = fastx_sets.random_input(rng)
        lay = ca.fastx_scan_host(data)
        assert lay.accepted == fastx_sets.in_regular_class(data), (k, data, lay.decline_reason, lay.decline_pos)
        if lay.accepted:
            accepted += 1
            check_against_kseq(ca, tmp_path, data, (k, data))
        else:
            assert 1 <= lay.decline_reason <= 10 and lay.decline_pos <= len(data), (k, data)
    assert accepted >= 0.8 * n, accepted
