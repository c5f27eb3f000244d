"""Plain gzip on the host (crass_gzip_inflate_host, crass_amd/csrc/gunzip.cpp): the serial run of the chunk rule the kernels run
(gunzip_core.h) against zlib — the text of every regular file at every chunk size, the stated reason of every declined file,
bit flips (accepted only where zlib accepts, with zlib's text), the plan of sets whose chain must really be made of many chunks,
the overflow protocol and the argument errors.  No GPU needed."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import gzip_sets

REGULAR = gzip_sets.regular()
DECLINED = gzip_sets.declined()
NEW_SYMBOLS = ["crass_gzip_inflate_host", "crass_gzip_plan_free", "crass_hip_inflate_gzip_device", "crass_hip_load_fastx_gzip",
               "crass_hip_set_gzip_on_device", "crass_hip_last_gzip_ms"]
# the smallest of 4096 / 16384 / 65536 at which the chain holds at least half of at least 8 chunks, chosen on the CPU per set
CHAIN_CHUNK = {"fastq_level_6": 65536, "fasta_level_6": 65536, "short_blocks": 4096}
NONE = 2 ** 64 - 1


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def test_symbols(ca):
    lib = C.CDLL(ca.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in ca.SYMBOLS and hasattr(lib, name), name


def test_the_sets_are_what_they_say():
    for name, (data, text) in REGULAR.items():
        assert zlib.decompress(data, 31) == text, name
        assert data[:3] == b"\x1f\x8b\x08" and len(data) < 1100000, name
    assert zlib.decompress(REGULAR["header_all_four"][0], 31) == REGULAR["header_all_four"][1]
    assert len(REGULAR["random_block_repeated"][1]) == 32768 + 258 * 400 * 40


@pytest.mark.parametrize("name", sorted(REGULAR))
def test_text_is_zlibs_at_every_chunk_size(ca, name):
    data, text = REGULAR[name]
    want = np.frombuffer(zlib.decompress(data, 31), np.uint8)
    for chunk in gzip_sets.CHUNKS:
        got, plan = ca.gzip_inflate_host(data, chunk, with_plan=True)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, chunk)
        dn = len(data) - 8 - 10          # (at most: a longer header leaves less)
        assert 1 <= plan.n_chain <= plan.n_chunks <= max(1, dn // (chunk or 262144)), (name, chunk)
        # the chain, restated: from chunk 0 along link to END, its lengths sum to the text's
        k, n, total = 0, 0, 0
        while True:
            assert plan.start_bit[k] != NONE
            n, total = n + 1, total + int(plan.text_len[k])
            if plan.link[k] == ca.GzipPlan.LINK_END:
                break
            assert k < plan.link[k] < plan.n_chunks, (name, chunk, k)
            k = int(plan.link[k])
        assert (n, total) == (plan.n_chain, len(text)), (name, chunk)
        assert plan.start_bit[0] == 0


@pytest.mark.parametrize("name", sorted(CHAIN_CHUNK))
def test_the_chunking_really_happens(ca, name):
    """a run in which chunk 0 decodes everything shows nothing: at the pinned chunk size at least half of at least 8 chunks are
    chain elements, and no smaller size of the three does that"""
    assert name in gzip_sets.chained()
    data, text = REGULAR[name]
    for chunk in (4096, 16384, 65536):
        plan = ca.gzip_inflate_host(data, chunk, with_plan=True)[1]
        good = plan.n_chunks >= 8 and 2 * plan.n_chain >= plan.n_chunks
        print(name, chunk, plan.n_chunks, plan.n_chain)
        if chunk == CHAIN_CHUNK[name]:
            assert good, (name, chunk, plan.n_chunks, plan.n_chain)
            break
        assert not good, (name, chunk, plan.n_chunks, plan.n_chain)


def test_short_blocks_chain_chunks_are_shorter_than_a_window(ca):
    """several consecutive chain elements shorter than 32 KB, so that a window shows text from two and three chunks back"""
    plan = ca.gzip_inflate_host(REGULAR["short_blocks"][0], 4096, with_plan=True)[1]
    lens = [int(plan.text_len[k]) for k in range(plan.n_chunks) if plan.link[k] < ca.GzipPlan.LINK_NONE or plan.link[k] == ca.GzipPlan.LINK_END]
    assert plan.n_chain == plan.n_chunks == len(lens) and max(lens) < 16000
    assert any(a + b + c < 32768 for a, b, c in zip(lens, lens[1:], lens[2:]))


def test_false_starts_are_off_the_chain(ca):
    """the deflate stream inside stored blocks has block starts that pass the whole test: chunks find them, the chain never lands on them"""
    data, text = REGULAR["embedded_stream_in_stored_blocks"]
    plan = ca.gzip_inflate_host(data, 4096, with_plan=True)[1]
    on, k = set(), 0
    while True:
        on.add(k)
        if plan.link[k] == ca.GzipPlan.LINK_END:
            break
        k = int(plan.link[k])
    off = [k for k in range(plan.n_chunks) if plan.start_bit[k] != NONE and k not in on]
    assert off, "no chunk found a start that the chain passes by"


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_files_give_their_reason(ca, name):
    data, chunk, reason = DECLINED[name]
    with pytest.raises(ca.BgzfDeclined) as e:
        ca.gzip_inflate_host(data, chunk)
    assert e.value.status == 2 and e.value.reason == reason, (name, e.value.verdict, reason)
    if reason in (gzip_sets.NOT_GZIP, gzip_sets.CRC, gzip_sets.OUTPUT_LONG, gzip_sets.OUTPUT_SHORT):
        assert e.value.verdict == (reason, 0, 0)
    else:
        k = e.value.member
        assert e.value.in_pos == 10 + int(e.value.plan.start_bit[k]) // 8, name      # (these files have the 10-byte header)


def test_the_span_inputs_are_accepted_at_a_chunk_where_they_fit(ca):
    for name, (data, chunk, text) in gzip_sets.accepted_at_a_larger_chunk().items():
        assert zlib.decompress(data, 31) == text
        assert ca.gzip_inflate_host(data, chunk).tobytes() == text, name


def test_single_bit_flips(ca):
    """a flipped file is declined, or accepted with exactly what zlib gives for the same bytes: never a different answer"""
    declined = 0
    for i, data in enumerate(gzip_sets.bit_flips()):
        try:
            got = ca.gzip_inflate_host(data, gzip_sets.FLIP_CHUNK).tobytes()
        except ca.BgzfDeclined as e:
            assert 1 <= e.reason <= 14 and e.status == 2
            declined += 1
            continue
        assert zlib.decompress(data, 31) == got, i      # (zlib raising here fails the test too)
    assert declined >= 150


def test_overflow_protocol_and_argument_errors(ca):
    lib = ca.load()
    data, text = REGULAR["fasta_level_9"]
    a = np.frombuffer(data, np.uint8)
    n_text, ver = C.c_uint64(7), ca._abi.BgzfVerdict()
    out = np.full(len(text) + 64, 0xA7, np.uint8)
    # one byte short: the size is reported, nothing is written
    assert lib.crass_gzip_inflate_host(a.ctypes.data, len(a), 16384, out.ctypes.data, len(text) - 1, C.byref(n_text), None, C.byref(ver)) == 8
    assert n_text.value == len(text) and bool(np.all(out == 0xA7)) and ver.reason == 0
    with pytest.raises(ca.CrassError) as e:
        ca.gzip_inflate_host(data, 16384, out_cap=len(text) - 1)
    assert e.value.status == 8 and e.value.n_text == len(text) and not e.value.out.any()
    # the size query, then exactly enough
    assert lib.crass_gzip_inflate_host(a.ctypes.data, len(a), 16384, None, 0, C.byref(n_text), None, None) == 8 and n_text.value == len(text)
    assert lib.crass_gzip_inflate_host(a.ctypes.data, len(a), 16384, out.ctypes.data, len(text), C.byref(n_text), None, None) == 0
    assert out[:len(text)].tobytes() == text and bool(np.all(out[len(text):] == 0xA7))
    # argument errors
    assert lib.crass_gzip_inflate_host(a.ctypes.data, len(a), 0, out.ctypes.data, len(out), None, None, None) == 1
    assert lib.crass_gzip_inflate_host(None, len(a), 0, out.ctypes.data, len(out), C.byref(n_text), None, None) == 1
    assert lib.crass_gzip_inflate_host(a.ctypes.data, len(a), 0, None, len(out), C.byref(n_text), None, None) == 1
    # no bytes at all: not a gzip header
    assert lib.crass_gzip_inflate_host(None, 0, 0, None, 0, C.byref(n_text), None, C.byref(ver)) == 2 and ver.reason == gzip_sets.NOT_GZIP
    # a chunk size below the floor is the floor
    p1 = ca.gzip_inflate_host(data, 1, with_plan=True)[1]
    p2 = ca.gzip_inflate_host(data, 4096, with_plan=True)[1]
    assert p1.n_chunks == p2.n_chunks and np.array_equal(p1.start_bit, p2.start_bit)
