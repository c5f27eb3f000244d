"""The scratch contract of the device ingest calls: what a call allocates for itself on the device goes back on every way out.
crassi_dev_bytes_live() (an internal export, not in crass_hip.h) is the byte count the library's device buffers keep; every
comparison is exact equality of that count, or "not more than before".

The input is 64 reads of 100 bases with a header each (a FASTQ file of about 14 KB), so every case is far under a second.  The
load routes take no chunk size (a plain gzip file of this size is one chunk there); the gzip scratch of a file of SEVERAL chunks
is pinned through crass_hip_inflate_gzip_device / _members_device at 4096-byte chunks on a text of about 80 KB, as
tests/gzip_sets.py does."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from tests import bgzf_sets, gzip_sets

pytestmark = pytest.mark.gpu

PAD = 2
N_READS, READ_LEN = 64, 100


def make_reads(n, seed=7):
    rng = np.random.RandomState(seed)
    return [np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, READ_LEN)].tobytes() for _ in range(n)]


def make_fastq(reads, prefix=b"r"):
    return b"".join(b"@%s%d lane=%d\n%s\n+\n%s\n" % (prefix, i, i % 4, s, b"F" * len(s)) for i, s in enumerate(reads))


READS = make_reads(N_READS)
FQ = make_fastq(READS)
FQ_B = make_fastq(make_reads(N_READS, seed=8), prefix=b"s")
HALF = FQ.index(b"@r32 ")
REC_POS = np.array([FQ.index(b"@r%d " % i) for i in range(N_READS)] + [len(FQ)], np.uint64)
PICK = [0, 63, 5, 5, 31]
BGZF = bgzf_sets.bgzf(FQ, block=3000)                            # five members and the EOF member
GZ = gzip_sets.gz(FQ)
GZ_MEMBERS = gzip_sets.gz(FQ[:HALF]) + gzip_sets.gz(FQ[HALF:])
# the text of several chunks: a Z_BLOCK flush every 3 000 text bytes, so that every 4096-byte chunk holds a block start
CHUNK = 4096
LONG_TEXT = gzip_sets.fastq(61, 80000)
LONG_GZ = gzip_sets.gz(LONG_TEXT, flushes=[(p, zlib.Z_BLOCK) for p in range(3000, len(LONG_TEXT), 3000)])
LONG_GZ_MEMBERS = LONG_GZ + gzip_sets.gz(LONG_TEXT[:5000])


def short_quality():
    """FQ with the quality line of record 10 one byte short"""
    at = FQ.index(b"@r11 ") - 2
    assert FQ[at:at + 2] == b"F\n"
    return FQ[:at] + FQ[at + 1:]


def damaged_bgzf():
    """BGZF with the CRC-32 of its second member wrong: the index is fine, the inflate kernel declines the member"""
    ms = [bytearray(bgzf_sets.member(FQ[i:i + 3000])) for i in range(0, len(FQ), 3000)]
    ms[1][-8] ^= 1
    return b"".join(bytes(m) for m in ms) + bgzf_sets.EOF


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def live(ca):
    lib = ca.load()
    lib.crassi_dev_bytes_live.restype = C.c_uint64
    lib.crassi_dev_bytes_live.argtypes = []
    return lambda: int(lib.crassi_dev_bytes_live())


@pytest.fixture(scope="module")
def dev(ca):
    """the inputs that live on the device (torch's memory: none of it is in the library's count), and the index of BGZF"""
    with ca.SearchEngine():                                      # (the library's HIP runtime comes up first, as in the other GPU tests:
        pass                                                     # behind torch's, crass_hip_create finds no device)
    import torch
    t = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    return {"fq": t(FQ), "long_gz": t(LONG_GZ), "long_gz_members": t(LONG_GZ_MEMBERS), "bgzf": t(BGZF), "bgzf_index": ca.engine.bgzf_index(BGZF),
            "out": torch.zeros(len(LONG_TEXT) + 5000 + 64, dtype=torch.uint8, device="cuda")}


LOADS = {
    "load_fastx_bytes": lambda e, d: e.load_fastx_bytes(FQ, pad_uniform=PAD),
    "attach_device_fastx": lambda e, d: e.attach_device_fastx(d["fq"], pad_uniform=PAD),
    "load_fastx_bgzf": lambda e, d: e.load_fastx_bgzf(BGZF, pad_uniform=PAD),
    "load_fastx_gzip": lambda e, d: e.load_fastx_gzip(GZ, pad_uniform=PAD),
    "load_fastx_gzip_members": lambda e, d: e.load_fastx_gzip_members(GZ_MEMBERS, pad_uniform=PAD),
}


def test_the_inputs_are_what_they_say(ca):
    lay = ca.fastx_scan_host(FQ)
    assert lay.accepted and lay.n_reads == N_READS and lay.max_len == READ_LEN and np.array_equal(lay.rec_pos, REC_POS)
    assert not ca.fastx_scan_host(short_quality()).accepted
    n_members = -(-len(FQ) // 3000) + 1                          # (and the EOF member)
    assert n_members >= 4 and ca.engine.bgzf_index(BGZF).n_members == n_members == ca.engine.bgzf_index(damaged_bgzf()).n_members
    with pytest.raises(ca.engine.BgzfDeclined):
        ca.engine.bgzf_inflate_host(damaged_bgzf())
    text, plan = ca.engine.gzip_inflate_host(LONG_GZ, chunk_bytes=CHUNK, with_plan=True)
    assert text.tobytes() == LONG_TEXT and plan.n_chunks >= 3 and plan.n_chain >= 3
    text, plan, members = ca.engine.gzip_inflate_members_host(LONG_GZ_MEMBERS, chunk_bytes=CHUNK, with_plan=True)
    assert text.tobytes() == LONG_TEXT + LONG_TEXT[:5000] and plan.n_chunks >= 3 and members.n_members == 2


def test_an_accepted_load_keeps_what_load_text_keeps(ca, live, dev):
    """one context throughout, so the pass-1 / pass-2 scratch sized at load is the same after every route"""
    with ca.SearchEngine() as e:
        e.load_text(READS, pad_uniform=PAD)
        want = live()
        for name, route in LOADS.items():
            lay = route(e, dev)
            assert lay.n_reads == N_READS, name
            assert live() == want, name
        e.load_text(READS, pad_uniform=PAD)
        assert live() == want


def _two_files(e, d):
    return e.load_fastx_files([FQ, bgzf_sets.bgzf(FQ_B, block=3000)], pad_uniform=PAD)


def _names(e, d):
    e.names_build(d["fq"], REC_POS)
    first = e.names_find([b"r5", b"r63", b"nobody"])
    e.names_drop()
    return first


def _out(d, n):
    return d["out"][:n]


CALLS = dict(LOADS, **{
    "load_fastx_files": _two_files,
    "header_ids": lambda e, d: e.device_header_ids(d["fq"], REC_POS, install=False),
    "header_ids_installed": lambda e, d: e.device_header_ids(d["fq"], REC_POS, install=True),
    "header_lines": lambda e, d: e.fetch_header_lines(d["fq"], REC_POS, PICK),
    "header_lines_to": lambda e, d: e.fetch_header_lines(d["fq"], REC_POS, PICK, out=_out(d, 4096)),
    "quality": lambda e, d: e.fetch_quality(d["fq"], len(FQ), REC_POS, PICK),
    "quality_to": lambda e, d: e.fetch_quality(d["fq"], len(FQ), REC_POS, PICK, out=_out(d, 4096)),
    "names_build_find_drop": _names,
    "inflate_bgzf_device": lambda e, d: e.inflate_bgzf_device(d["bgzf"], d["bgzf_index"], _out(d, len(FQ))),
    "inflate_gzip_device_chunks": lambda e, d: e.inflate_gzip_device(d["long_gz"], d["out"], chunk_bytes=CHUNK),
    "inflate_gzip_members_device_chunks": lambda e, d: e.inflate_gzip_members_device(d["long_gz_members"], d["out"], chunk_bytes=CHUNK),
})


@pytest.mark.parametrize("name", sorted(CALLS))
def test_three_calls_in_a_row_leave_the_same(ca, live, dev, name):
    from crass_amd import _abi
    with ca.SearchEngine() as e:
        e.load_fastx_bytes(FQ, pad_uniform=PAD)                  # (a resident set of the same records: header_ids_installed needs one)
        after = []
        for _ in range(3):
            CALLS[name](e, dev)
            after.append(live())
        assert after[0] == after[1] == after[2], (name, after)
        if name == "names_build_find_drop":
            assert CALLS[name](e, dev).tolist() == [5, 63, _abi.NAME_NOT_FOUND]


def _declined_two_files(e, d):
    e.load_fastx_files([FQ, short_quality()], pad_uniform=PAD)


DECLINED = {
    "first_byte": lambda e, d: e.load_fastx_bytes(b"x" + FQ, pad_uniform=PAD),
    "quality_one_byte_short": lambda e, d: e.load_fastx_bytes(short_quality(), pad_uniform=PAD),
    "bgzf_damaged_member": lambda e, d: e.load_fastx_bgzf(damaged_bgzf(), pad_uniform=PAD),
    "second_of_two_files": _declined_two_files,
}


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_a_declined_load_gives_everything_back(ca, live, dev, name):
    with ca.SearchEngine() as e:
        e.load_text(READS, pad_uniform=PAD)
        want = live()
        e.load_fastx_bytes(FQ, pad_uniform=PAD)                  # something is resident
        before = live()
        after = []
        for _ in range(2):
            with pytest.raises(ca.CrassError) as ei:
                DECLINED[name](e, dev)
            assert ei.value.status == 2, name
            after.append(live())
        assert after[0] == after[1], (name, after)
        assert after[0] <= before, (name, after, before)
        with pytest.raises(ca.CrassError) as ei:                 # nothing resident
            e.seed_scan()
        assert ei.value.status == 6
        lay = e.load_fastx_bytes(FQ, pad_uniform=PAD)            # the context takes a good load
        assert lay.n_reads == N_READS and live() == want == before, name
        e.seed_scan()


def test_out_of_memory_leaves_the_count_where_it_was(ca, live):
    big = make_fastq(make_reads(18000, seed=9))                  # about 4 MB of file bytes
    assert 3900000 < len(big) < 4300000
    os.environ["CRASS_POOL_CAP_MB"] = "1"
    capped = None
    try:
        capped = ca.SearchEngine()
        before = live()
        for _ in range(2):
            with pytest.raises(ca.CrassError) as ei:
                capped.load_fastx_bytes(big, pad_uniform=PAD)
            assert ei.value.status == 5                          # CRASS_ERR_OOM
            assert live() == before
        os.environ.pop("CRASS_POOL_CAP_MB")
        with ca.SearchEngine() as e:                             # a new context reads the environment again: no cap
            lay = e.load_fastx_bytes(big, pad_uniform=PAD)
            assert lay.n_reads == 18000
        assert live() == before
    finally:
        os.environ.pop("CRASS_POOL_CAP_MB", None)
        if capped is not None:
            capped.reload_env()                                  # (the cap is the process's: it must not outlive this test)
            capped.close()
