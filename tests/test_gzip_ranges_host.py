"""Plain gzip by ranges on the host (crass_gzip_inflate_ranges_host, crass_amd/csrc/gunzip.cpp): the rule the ranks of a group run
(chain elements dealt over text ranges, symbolic windows from an identity entry, the entry windows composed in order,
gunzip_core.h) as a serial run, against zlib and against crass_gzip_inflate_host: the text of every regular file at every chunk
size and number of ranges, cuts designed around the chain's element boundaries on the sets whose windows chain through every
element, the verdict of declined and damaged files field for field, and the shards of a job whose gzip files are taken as
their text (crass_fastx_files_shards_host_gzip).  No GPU needed."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import group_gzip_sets as ggs
from tests import gzip_sets

REGULAR = gzip_sets.regular()
DECLINED = gzip_sets.declined()
NEW_SYMBOLS = ["crass_gzip_inflate_ranges_host", "crass_fastx_files_shards_host_gzip", "crass_hip_group_inflate_gzip",
               "crass_hip_group_gzip_counters", "crass_hip_group_gzip_ms"]


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def plan_tuple(p):
    return (p.n_chunks, p.n_chain, p.start_bit.tolist(), p.link.tolist(), p.text_len.tolist())


def test_symbols_and_header(ca):
    lib = C.CDLL(ca.LIB_PATH)
    header = open(ca.LIB_PATH.replace("crass_amd/libcrass_hip.so", "include/crass_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in ca.SYMBOLS and hasattr(lib, name) and name + "(" in header, name


@pytest.mark.parametrize("name", sorted(REGULAR))
def test_text_is_zlibs_for_every_chunk_and_number_of_ranges(ca, name):
    assert set(gzip_sets.chained()) <= set(REGULAR)
    data, text = REGULAR[name]
    want = np.frombuffer(zlib.decompress(data, 31), np.uint8)
    assert want.tobytes() == text
    for chunk in gzip_sets.CHUNKS:
        want_plan = plan_tuple(ca.gzip_inflate_host(data, chunk, with_plan=True)[1])
        for n in ggs.N_RANGES:
            got, plan = ca.gzip_inflate_ranges_host(data, n, chunk, with_plan=True)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, chunk, n)
            assert plan_tuple(plan) == want_plan, (name, chunk, n)


@pytest.mark.parametrize("name", ["short_blocks", "random_block_repeated"])
def test_cuts_around_element_boundaries(ca, name):
    """the sets whose windows show text from several elements back (short_blocks) and whose every byte is copied from the element
    before (distance 32 768): a wrong entry, a wrong composition or an element left out changes the text"""
    data, text = REGULAR[name]
    want, plan = ca.gzip_inflate_host(data, ggs.CUT_CHUNK, with_plan=True)
    assert want.tobytes() == text
    off = ggs.chain_offsets(plan)
    assert len(off) - 1 >= 8
    cuts = dict(ggs.boundary_cuts(off))
    for n in (2, 3, 4):
        for k, v in ggs.empty_and_crowded_cuts(off, n).items():
            cuts["%s_%d" % (k, n)] = v
    for what, nominal in sorted(cuts.items()):
        got, p = ca.gzip_inflate_ranges_host(data, len(nominal) + 1, ggs.CUT_CHUNK, nominal=nominal, with_plan=True)
        assert np.array_equal(got, want), (name, what, nominal)
        assert plan_tuple(p) == plan_tuple(plan), (name, what)


def verdict_of(ca, fn):
    try:
        fn()
    except ca.BgzfDeclined as e:
        return e.verdict, plan_tuple(e.plan)
    return None, None


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_files_give_the_host_functions_verdict(ca, name):
    data, chunk, reason = DECLINED[name]
    want = verdict_of(ca, lambda: ca.gzip_inflate_host(data, chunk))
    assert want[0] is not None and want[0][0] == reason
    for n in (2, 3):
        assert verdict_of(ca, lambda: ca.gzip_inflate_ranges_host(data, n, chunk)) == want, (name, n)


def test_single_bit_flips_give_the_host_functions_answer(ca):
    declined, reasons = 0, set()
    for i, data in enumerate(gzip_sets.bit_flips()[:50]):
        want = verdict_of(ca, lambda: ca.gzip_inflate_host(data, gzip_sets.FLIP_CHUNK))
        for n in (2, 3):
            got = verdict_of(ca, lambda: ca.gzip_inflate_ranges_host(data, n, gzip_sets.FLIP_CHUNK))
            assert got == want, (i, n, got[0], want[0])
            if want[0] is None:
                assert ca.gzip_inflate_ranges_host(data, n, gzip_sets.FLIP_CHUNK).tobytes() == zlib.decompress(data, 31), (i, n)
        declined += want[0] is not None
        reasons.add(want[0][0] if want[0] else 0)
    assert declined >= 35 and len(reasons) >= 3, (declined, reasons)


def test_overflow_protocol_and_argument_errors(ca):
    lib = ca.load()
    data, text = REGULAR["fasta_level_9"]
    a = np.frombuffer(data, np.uint8)
    n_text, ver = C.c_uint64(7), ca._abi.BgzfVerdict()
    out = np.full(len(text) + 64, 0xA7, np.uint8)
    f = lib.crass_gzip_inflate_ranges_host
    assert f(a.ctypes.data, len(a), 16384, 3, None, out.ctypes.data, len(text) - 1, C.byref(n_text), None, C.byref(ver)) == 8
    assert n_text.value == len(text) and bool(np.all(out == 0xA7)) and ver.reason == 0
    assert f(a.ctypes.data, len(a), 16384, 3, None, None, 0, C.byref(n_text), None, None) == 8 and n_text.value == len(text)
    assert f(a.ctypes.data, len(a), 16384, 3, None, out.ctypes.data, len(text), C.byref(n_text), None, None) == 0
    assert out[:len(text)].tobytes() == text and bool(np.all(out[len(text):] == 0xA7))
    for n in (0, 65):
        assert f(a.ctypes.data, len(a), 16384, n, None, out.ctypes.data, len(out), C.byref(n_text), None, None) == 1
    assert f(a.ctypes.data, len(a), 16384, 2, None, out.ctypes.data, len(out), None, None, None) == 1
    assert f(None, len(a), 16384, 2, None, out.ctypes.data, len(out), C.byref(n_text), None, None) == 1
    for nominal in ([len(text) + 1], [5, 4]):
        nom = ggs.as_u64(nominal)
        assert f(a.ctypes.data, len(a), 16384, len(nominal) + 1, nom.ctypes.data, out.ctypes.data, len(out), C.byref(n_text), None, None) == 1, nominal


# ---- the shards of a job whose gzip files are taken as their text ----
def same_shards(a, b):
    assert a.verdict == b.verdict and (a.n_ranks, a.n_files, a.n_reads, a.max_len) == (b.n_ranks, b.n_files, b.n_reads, b.max_len)
    for k in ("rank_read_base", "cut_file", "cut_pos", "file_read_base"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.formats == b.formats


def test_shards_of_a_job_with_a_gzip_file(ca):
    fq, fa = gzip_sets.fastq(91, 300000), gzip_sets.fasta(92, 80000)
    zipped = gzip_sets.gz(fq)
    for n_ranks in (1, 2, 3, 4):
        got = ca.fastx_files_shards_host_gzip([zipped, fa], n_ranks, gzip_mode=1)
        want = ca.fastx_files_shards_host([fq, fa], n_ranks)
        assert got.accepted and got.n_reads > 0
        same_shards(got, want)
        # mode 0: the existing function on the same bytes, the decline included
        off = ca.fastx_files_shards_host_gzip([zipped, fa], n_ranks, gzip_mode=0)
        today = ca.fastx_files_shards_host([zipped, fa], n_ranks)
        assert not off.accepted and off.verdict == (0, 0, 0, (gzip_sets.NOT_BGZF, 0, 0))
        same_shards(off, today)
    nominal = [len(fq) // 3, len(fq) + 100]
    same_shards(ca.fastx_files_shards_host_gzip([zipped, fa], 3, nominal=nominal), ca.fastx_files_shards_host([fq, fa], 3, nominal=nominal))
    same_shards(ca.fastx_files_shards_host_gzip([zipped, fa], 3, fastq_class=1), ca.fastx_files_shards_host([fq, fa], 3, fastq_class=1))


def test_shards_declines_in_file_order(ca):
    fq, fa = gzip_sets.fastq(93, 60000), gzip_sets.fasta(94, 30000)
    bad = bytearray(gzip_sets.gz(fq)); bad[-7] ^= 0x40
    two = DECLINED["two_members"][0]
    # a gzip file that does not inflate: its verdict is crass_gzip_inflate_host's
    d = ca.fastx_files_shards_host_gzip([fa, bytes(bad)], 2)
    assert not d.accepted and d.verdict == (1, 0, 0, (gzip_sets.CRC, 0, 0))
    d = ca.fastx_files_shards_host_gzip([fa, two, fq], 2)
    want = verdict_of(ca, lambda: ca.gzip_inflate_host(two, 0))[0]
    assert want[0] == gzip_sets.TRAILING and d.verdict == (1, 0, 0, want)
    # ... unless a file in front of it is declined
    irregular = b"@a\nACGT\n+\nIIII\n@b\nAC>T\n+\nIIII\n"
    d = ca.fastx_files_shards_host_gzip([irregular, bytes(bad)], 2)
    assert d.verdict == ca.fastx_files_shards_host([irregular], 2).verdict and d.decline_file == 0
    # the text of a gzip file is judged like any other
    d = ca.fastx_files_shards_host_gzip([fa, gzip_sets.gz(irregular)], 2)
    w = ca.fastx_files_shards_host([fa, irregular], 2)
    assert not d.accepted and d.verdict == w.verdict and d.decline_file == 1
