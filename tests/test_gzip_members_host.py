"""Plain gzip of several members on the host (crass_gzip_inflate_members_host, crass_amd/csrc/gunzip.cpp): the serial run of the
chunk rule in members mode (gunzip_core.h) against the strict zlib loop — the text and the member table of every regular file at
every chunk size, the stated reason and fields of every declined file (zlib raises on each), bit flips (accepted only where the
strict loop accepts, with its text), member starts as chunk starts, starts the chain passes by, the single-member call's unchanged
decline, the overflow protocol and the argument errors.  No GPU needed."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import gzip_member_sets as sets
from tests import gzip_sets

REGULAR = sets.regular()
DECLINED, OFFS = sets.declined()
NEW_SYMBOLS = ["crass_gzip_inflate_members_host", "crass_gzip_members_free", "crass_hip_inflate_gzip_members_device",
               "crass_hip_load_fastx_gzip_members"]
NONE = 2 ** 64 - 1


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def on_chain(ca, plan):
    on, k = [], 0
    while True:
        on.append(k)
        if plan.link[k] == ca.GzipPlan.LINK_END:
            return on
        assert k < plan.link[k] < plan.n_chunks
        k = int(plan.link[k])


def test_symbols(ca):
    lib = C.CDLL(ca.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in ca.SYMBOLS and hasattr(lib, name), name


def test_the_sets_are_what_they_say():
    for name, data in REGULAR.items():
        text, in_off, text_off = sets.strict(data)
        assert data[:3] == b"\x1f\x8b\x08" and len(data) < 1100000 and in_off[-1] == len(data), name
        print(name, len(data), len(data) // 4096, len(in_off) - 1, len(text))
    assert len(sets.strict(REGULAR["three_big_members"])[1]) == 4 and len(sets.strict(REGULAR["many_single_block_members"])[1]) == 121
    assert len(sets.EMPTY) == 20 and REGULAR["empty_members_everywhere"].startswith(sets.EMPTY) and REGULAR["empty_members_everywhere"].endswith(sets.EMPTY)
    assert REGULAR["one_member"] == gzip_sets.gz(gzip_sets.fasta(12, 2400000)[:1200000], level=9)
    assert sets.member_inside_stored_block()[1] in sets.strict(REGULAR["member_inside_stored_block"])[0]
    for name, (data, text) in sets.fastx_members().items():
        assert sets.strict(data)[0] == text, name
    # zlib raises on every declined file
    for name, (data, chunk, reason, member) in DECLINED.items():
        with pytest.raises(zlib.error):
            sets.strict(data)
    # ... and alone rejects at least three quarters of the flips
    rejected = 0
    for data in sets.bit_flips():
        try:
            sets.strict(data)
        except zlib.error:
            rejected += 1
    assert rejected >= 300, rejected


@pytest.mark.parametrize("name", sorted(REGULAR))
def test_text_and_members_are_zlibs_at_every_chunk_size(ca, name):
    data = REGULAR[name]
    text, in_off, text_off = sets.strict(data)
    want = np.frombuffer(text, np.uint8)
    for chunk in sets.CHUNKS:
        got, plan, members = ca.gzip_inflate_members_host(data, chunk, with_plan=True)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, chunk)
        assert members.n_members == len(in_off) - 1, (name, chunk)
        assert members.in_off.tolist() == in_off and members.text_off.tolist() == text_off, (name, chunk)
        chain = on_chain(ca, plan)
        assert len(chain) == plan.n_chain and sum(int(plan.text_len[k]) for k in chain) == len(text), (name, chunk)
        assert plan.start_bit[0] == 0 and all(plan.start_bit[k] != NONE for k in chain)


def test_one_member_gives_the_single_member_plan(ca):
    data = REGULAR["one_member"]
    for chunk in sets.CHUNKS:
        a = ca.gzip_inflate_host(data, chunk, with_plan=True)[1]
        b = ca.gzip_inflate_members_host(data, chunk, with_plan=True)[1]
        assert (a.n_chunks, a.n_chain) == (b.n_chunks, b.n_chain), chunk
        assert np.array_equal(a.start_bit, b.start_bit) and np.array_equal(a.link, b.link) and np.array_equal(a.text_len, b.text_len), chunk


def test_member_starts_are_chunk_starts(ca):
    """members of one final block each have no block start the single-member test takes: the chain is made of header starts"""
    data = REGULAR["many_single_block_members"]
    plan = ca.gzip_inflate_members_host(data, 4096, with_plan=True)[1]
    chain = on_chain(ca, plan)
    print(plan.n_chunks, plan.n_chain)
    assert plan.n_chunks >= 150 and 2 * plan.n_chain >= plan.n_chunks
    for k in chain[1:]:
        bit = int(plan.start_bit[k])
        assert bit % 8 == 0 and data[10 + bit // 8:10 + bit // 8 + 3] == b"\x1f\x8b\x08", k
    # the single-member call goes on declining the file
    with pytest.raises(ca.BgzfDeclined) as e:
        ca.gzip_inflate_host(data, 4096)
    assert e.value.reason == sets.TRAILING


def test_false_starts_are_off_the_chain(ca):
    data = REGULAR["member_inside_stored_block"]
    inner = sets.member_inside_stored_block()[1]
    at = data.index(inner)
    plan = ca.gzip_inflate_members_host(data, 4096, with_plan=True)[1]
    chain = set(on_chain(ca, plan))
    off = [k for k in range(plan.n_chunks) if plan.start_bit[k] != NONE and k not in chain]
    assert off, "no chunk found a start that the chain passes by"
    inside = [k for k in off if at <= 10 + int(plan.start_bit[k]) // 8 < at + len(inner)]
    assert inside and all(k not in chain for k in inside)


def test_short_block_boundary_has_elements_behind_it(ca):
    """chain elements start a few KB behind the member boundary: their windows show the previous member's text"""
    data = REGULAR["boundary_in_short_blocks"]
    _, in_off, _ = sets.strict(data)
    plan = ca.gzip_inflate_members_host(data, 4096, with_plan=True)[1]
    chain = on_chain(ca, plan)
    starts = [10 + int(plan.start_bit[k]) // 8 for k in chain]
    assert any(in_off[1] < s < in_off[1] + 8192 for s in starts)


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_files_give_their_reason_and_fields(ca, name):
    data, chunk, reason, member = DECLINED[name]
    with pytest.raises(ca.BgzfDeclined) as e:
        ca.gzip_inflate_members_host(data, chunk)
    assert e.value.status == 2 and e.value.reason == reason, (name, e.value.verdict, reason)
    if member is not None:
        assert e.value.verdict == (reason, member, OFFS[member]), (name, e.value.verdict)
    else:
        k = e.value.member
        assert e.value.in_pos == 10 + int(e.value.plan.start_bit[k]) // 8, name      # (these files begin with the 10-byte header)
    if name == "distance_over_the_boundary_in_narrowing":
        # (the element begins on a block start inside the hand-made member, not on a member start: the marker is narrowing's to refuse)
        assert e.value.member > 0 and int(e.value.plan.start_bit[e.value.member]) % 8 != 0 and e.value.in_pos > len(data) - 13000
    if name == "distance_over_the_boundary_in_a_run":
        assert e.value.plan.n_chunks == 1 and e.value.member == 0


def test_the_first_header_declines_as_member_0(ca):
    good = REGULAR["three_big_members"]
    for data in (b"", good[:3], b"\x1f\x8b\x07" + good[3:], good[:3] + b"\x20" + good[4:]):
        with pytest.raises(ca.BgzfDeclined) as e:
            ca.gzip_inflate_members_host(data, 4096)
        assert e.value.verdict == (sets.NOT_GZIP, 0, 0)


def test_single_bit_flips(ca):
    """a flipped file is declined, or accepted with exactly what the strict zlib loop gives for the same bytes"""
    declined = 0
    for i, data in enumerate(sets.bit_flips()):
        try:
            got = ca.gzip_inflate_members_host(data, sets.FLIP_CHUNK).tobytes()
        except ca.BgzfDeclined as e:
            assert 1 <= e.reason <= 14 and e.status == 2
            declined += 1
            continue
        assert sets.strict(data)[0] == got, i            # (zlib raising here fails the test too)
    assert declined >= 300


def test_overflow_protocol_and_argument_errors(ca):
    lib = ca.load()
    data = REGULAR["inner_headers_all_four"]
    text = sets.strict(data)[0]
    a = np.frombuffer(data, np.uint8)
    n_text, ver = C.c_uint64(7), ca._abi.BgzfVerdict()
    fn = lib.crass_gzip_inflate_members_host
    out = np.full(len(text) + 64, 0xA7, np.uint8)
    assert fn(a.ctypes.data, len(a), 16384, out.ctypes.data, len(text) - 1, C.byref(n_text), None, None, C.byref(ver)) == 8
    assert n_text.value == len(text) and bool(np.all(out == 0xA7)) and ver.reason == 0
    with pytest.raises(ca.CrassError) as e:
        ca.gzip_inflate_members_host(data, 16384, out_cap=len(text) - 1)
    assert e.value.status == 8 and e.value.n_text == len(text) and not e.value.out.any()
    assert fn(a.ctypes.data, len(a), 16384, None, 0, C.byref(n_text), None, None, None) == 8 and n_text.value == len(text)
    mc = ca._abi.GzipMembersC()
    assert fn(a.ctypes.data, len(a), 16384, out.ctypes.data, len(text), C.byref(n_text), None, C.byref(mc), None) == 0
    assert mc.n_members == 3 and mc.in_off[3] == len(data) and mc.text_off[3] == len(text)
    lib.crass_gzip_members_free(C.byref(mc))
    assert mc.n_members == 0 and not mc.in_off and not mc.text_off
    lib.crass_gzip_members_free(C.byref(mc))             # (twice, and NULL: nothing)
    lib.crass_gzip_members_free(None)
    assert out[:len(text)].tobytes() == text and bool(np.all(out[len(text):] == 0xA7))
    assert fn(a.ctypes.data, len(a), 0, out.ctypes.data, len(out), None, None, None, None) == 1
    assert fn(None, len(a), 0, out.ctypes.data, len(out), C.byref(n_text), None, None, None) == 1
    assert fn(a.ctypes.data, len(a), 0, None, len(out), C.byref(n_text), None, None, None) == 1
    assert fn(None, 0, 0, None, 0, C.byref(n_text), None, None, C.byref(ver)) == 2 and ver.reason == sets.NOT_GZIP
    p1 = ca.gzip_inflate_members_host(data, 1, with_plan=True)[1]
    p2 = ca.gzip_inflate_members_host(data, 4096, with_plan=True)[1]
    assert p1.n_chunks == p2.n_chunks and np.array_equal(p1.start_bit, p2.start_bit)
