"""Plain gzip of several members by ranges on the host (crass_gzip_inflate_members_ranges_host, crass_amd/csrc/gunzip.cpp): the
members rule as the ranks of a group run it — GzEnd records per range, symbolic windows with dead entries as 0, the members'
CRC-32 from pieces, the verdict behind all narrowing — as a serial run, against crass_gzip_inflate_members_host and the strict
zlib loop: text, plan and member table of every regular file for 1, 2, 3, 4 and 7 ranges, cuts designed around member boundaries,
the verdict of every declined file and of 400 single-bit flips, and the shards of a job whose gzip files have several members
(crass_fastx_files_shards_host_gzip with gzip_mode 2).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tests import group_gzip_member_sets as gms
from tests import gzip_member_sets as sets
from tests import gzip_sets

REGULAR = sets.regular()
FASTX = sets.fastx_members()
DECLINED, OFFS = sets.declined()
DESIGNED = gms.designed()
FILES = dict(REGULAR, designed=DESIGNED[0], **{"fastx_" + k: v[0] for k, v in FASTX.items()})


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def plan_tuple(p):
    return (p.n_chunks, p.n_chain, p.start_bit.tolist(), p.link.tolist(), p.text_len.tolist())


def members_tuple(m):
    return (m.n_members, m.in_off.tolist(), m.text_off.tolist())


def outcome(ca, fn):
    """('text', bytes, plan, members) or ('declined', verdict, plan)"""
    try:
        t, p, m = fn()
    except ca.BgzfDeclined as e:
        return ("declined", e.verdict, plan_tuple(e.plan))
    return ("text", t.tobytes(), plan_tuple(p), members_tuple(m))


def test_symbol_and_header(ca):
    lib = C.CDLL(ca.LIB_PATH)
    header = open(ca.LIB_PATH.replace("crass_amd/libcrass_hip.so", "include/crass_hip.h")).read()
    name = "crass_gzip_inflate_members_ranges_host"
    assert name in ca.SYMBOLS and hasattr(lib, name) and name + "(" in header


def test_the_designed_file_is_what_it_says(ca):
    data, text = DESIGNED
    assert sets.strict(data)[0] == text
    got, plan, members = ca.gzip_inflate_members_host(data, gms.CHUNK, with_plan=True)
    off = gms.check_designed(data, text, plan, members)
    assert got.tobytes() == text and off[-1] == len(text)
    assert ca.gzip_inflate_members_ranges_host(data, 1, gms.CHUNK).tobytes() == text
    cuts = gms.designed_cuts(off)
    assert len(cuts) > 60 and all(list(v) == sorted(v) and v[-1] <= len(text) for v in cuts.values())


@pytest.mark.parametrize("name", sorted(FILES))
def test_text_plan_and_members_for_every_number_of_ranges(ca, name):
    data = FILES[name]
    want = outcome(ca, lambda: ca.gzip_inflate_members_host(data, gms.CHUNK, with_plan=True))
    assert want[0] == "text" and want[1] == sets.strict(data)[0]
    for n in gms.N_RANGES:
        got = outcome(ca, lambda: ca.gzip_inflate_members_ranges_host(data, n, gms.CHUNK, with_plan=True))
        assert got == want, (name, n)


def test_designed_cuts_on_the_designed_file(ca):
    data, text = DESIGNED
    want = outcome(ca, lambda: ca.gzip_inflate_members_host(data, gms.CHUNK, with_plan=True))
    _, plan, members = ca.gzip_inflate_members_host(data, gms.CHUNK, with_plan=True)
    off = gms.check_designed(data, text, plan, members)
    for what, nominal in sorted(gms.designed_cuts(off).items()):
        got = outcome(ca, lambda: ca.gzip_inflate_members_ranges_host(data, len(nominal) + 1, gms.CHUNK, nominal=nominal, with_plan=True))
        assert got == want, (what, nominal)


@pytest.mark.parametrize("name", ["boundary_in_short_blocks", "many_single_block_members", "empty_members_everywhere"])
def test_cuts_around_element_boundaries(ca, name):
    data = REGULAR[name]
    want = outcome(ca, lambda: ca.gzip_inflate_members_host(data, gms.CHUNK, with_plan=True))
    off = gms.ggs.chain_offsets(ca.gzip_inflate_members_host(data, gms.CHUNK, with_plan=True)[1])
    # (empty_members_everywhere ends on an element without text: the cuts that leave ranges empty and crowd them only)
    cuts = dict(gms.ggs.boundary_cuts(off)) if name != "empty_members_everywhere" else {}
    for n in (2, 3, 4):
        for k, v in gms.ggs.empty_and_crowded_cuts(off, n).items():
            cuts["%s_%d" % (k, n)] = v
    for what, nominal in sorted(cuts.items()):
        got = outcome(ca, lambda: ca.gzip_inflate_members_ranges_host(data, len(nominal) + 1, gms.CHUNK, nominal=nominal, with_plan=True))
        assert got == want, (name, what, nominal)


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_files_give_the_serial_verdict(ca, name):
    data, chunk, reason, member = DECLINED[name]
    want = outcome(ca, lambda: ca.gzip_inflate_members_host(data, chunk, with_plan=True))
    assert want[0] == "declined" and want[1][0] == reason
    if member is not None:
        assert want[1] == (reason, member, OFFS[member])
    for n in gms.N_RANGES:
        assert outcome(ca, lambda: ca.gzip_inflate_members_ranges_host(data, n, chunk, with_plan=True)) == want, (name, n)


def test_single_bit_flips_give_the_serial_outcome(ca):
    flips = sets.bit_flips()
    assert len(flips) == 400
    kinds = {}
    for i, data in enumerate(flips):
        want = outcome(ca, lambda: ca.gzip_inflate_members_host(data, sets.FLIP_CHUNK, with_plan=True))
        for n in (2, 3):
            got = outcome(ca, lambda: ca.gzip_inflate_members_ranges_host(data, n, sets.FLIP_CHUNK, with_plan=True))
            assert got == want, (i, n, got[:2] if got[0] == "declined" else got[0], want[:2] if want[0] == "declined" else want[0])
        kinds[want[1][0] if want[0] == "declined" else 0] = kinds.get(want[1][0] if want[0] == "declined" else 0, 0) + 1
    print(kinds)
    assert sum(v for k, v in kinds.items() if k) >= 300 and len(kinds) >= 4, kinds


def test_overflow_protocol_and_argument_errors(ca):
    lib = ca.load()
    data = REGULAR["empty_members_everywhere"]
    text = sets.strict(data)[0]
    a = np.frombuffer(data, np.uint8)
    n_text, ver, mc = C.c_uint64(7), ca._abi.BgzfVerdict(), ca._abi.GzipMembersC()
    out = np.full(len(text) + 64, 0xA7, np.uint8)
    f = lib.crass_gzip_inflate_members_ranges_host
    assert f(a.ctypes.data, len(a), 4096, 3, None, out.ctypes.data, len(text) - 1, C.byref(n_text), None, C.byref(mc), C.byref(ver)) == 8
    assert n_text.value == len(text) and bool(np.all(out == 0xA7)) and ver.reason == 0 and mc.n_members == 0
    assert f(a.ctypes.data, len(a), 4096, 3, None, None, 0, C.byref(n_text), None, None, None) == 8 and n_text.value == len(text)
    assert f(a.ctypes.data, len(a), 4096, 3, None, out.ctypes.data, len(text), C.byref(n_text), None, None, None) == 0
    assert out[:len(text)].tobytes() == text and bool(np.all(out[len(text):] == 0xA7))
    for n in (0, 65):
        assert f(a.ctypes.data, len(a), 4096, n, None, out.ctypes.data, len(out), C.byref(n_text), None, None, None) == 1
    assert f(a.ctypes.data, len(a), 4096, 2, None, out.ctypes.data, len(out), None, None, None, None) == 1
    assert f(None, len(a), 4096, 2, None, out.ctypes.data, len(out), C.byref(n_text), None, None, None) == 1
    for nominal in ([len(text) + 1], [5, 4]):
        nom = np.asarray(nominal, np.uint64)
        assert f(a.ctypes.data, len(a), 4096, len(nominal) + 1, nom.ctypes.data, out.ctypes.data, len(out), C.byref(n_text), None, None, None) == 1, nominal
    # 64 ranges, more than most files have elements to give
    got = ca.gzip_inflate_members_ranges_host(data, 64, 4096)
    assert got.tobytes() == text


# ---- the shards of a job whose gzip files have several members ----
def same_shards(a, b):
    assert a.verdict == b.verdict and (a.n_ranks, a.n_files, a.n_reads, a.max_len) == (b.n_ranks, b.n_files, b.n_reads, b.max_len)
    for k in ("rank_read_base", "cut_file", "cut_pos", "file_read_base"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.formats == b.formats


@pytest.mark.parametrize("name", sorted(FASTX))
def test_shards_of_a_job_with_a_file_of_several_members(ca, name):
    data, text = FASTX[name]
    fa = gzip_sets.fasta(92, 80000)
    for n_ranks in (1, 2, 3, 4):
        got = ca.fastx_files_shards_host_gzip([data, fa], n_ranks, gzip_mode=2, chunk_bytes=gms.CHUNK)
        assert got.accepted and got.n_reads > 0
        same_shards(got, ca.fastx_files_shards_host([text, fa], n_ranks))
        one = ca.fastx_files_shards_host_gzip([data, fa], n_ranks, gzip_mode=1, chunk_bytes=gms.CHUNK)
        assert not one.accepted and one.verdict[0] == 0 and one.verdict[3][0] == gzip_sets.TRAILING


def test_shards_give_the_verdict_of_a_damaged_member(ca):
    fa = gzip_sets.fasta(94, 30000)
    for name in ("crc_byte_of_member_1", "isize_of_member_2_off_by_one"):
        data, chunk, reason, member = DECLINED[name]
        d = ca.fastx_files_shards_host_gzip([fa, data], 2, gzip_mode=2, chunk_bytes=chunk)
        assert not d.accepted and d.verdict == (1, 0, 0, (reason, member, OFFS[member])), (name, d.verdict)
        one = ca.fastx_files_shards_host_gzip([fa, data], 2, gzip_mode=1, chunk_bytes=chunk)
        assert one.verdict[0] == 1 and one.verdict[3][0] == gzip_sets.TRAILING
    # a single-member file: mode 2 gives what mode 1 gives
    fq = gzip_sets.fastq(91, 300000)
    same_shards(ca.fastx_files_shards_host_gzip([gzip_sets.gz(fq), fa], 3, gzip_mode=2), ca.fastx_files_shards_host_gzip([gzip_sets.gz(fq), fa], 3, gzip_mode=1))
