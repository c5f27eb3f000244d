"""Plain gzip files of SEVERAL members for the members tests (tests/test_gzip_members_host.py, tests/test_gpu_gzip_members.py,
tests/test_gpu_cli_gzip_members.py): what `cat a.gz b.gz`, gzip's `>>` and a compressor that starts a member every N records
write, and damaged files with the reason a decoder must report.  The text of a file is what the strict zlib loop gives
(decompressobj(31) repeated over unused_data until nothing is left).  At most about 1 MB of compressed bytes per file: at a chunk
of 4096 bytes that is 100 to 250 chunks.  Everything is seeded."""
import struct
import zlib

import numpy as np

from tests import bgzf_sets
from tests.gzip_sets import (BLOCK_TYPE, CRC, INPUT_END, MARKER, NO_START, NOT_GZIP, OUTPUT_LONG, OUTPUT_SHORT, TRAILING,      # noqa: F401
                             CHUNKS, far_matches, fasta, fastq, gz, raw, wrap)

FLIP_CHUNK = 4096
EMPTY = gz(b"")


def strict(data):
    """the strict zlib loop: (text, in_off, text_off) with one entry per member and the totals at the end; raises zlib.error on
    anything zlib does not take to its end, trailing bytes that are no member included"""
    texts, in_off, text_off, at, total = [], [0], [0], 0, 0
    if not data:
        raise zlib.error("no member at all")
    while at < len(data):
        d = zlib.decompressobj(31)
        t = d.decompress(data[at:])
        if not d.eof:
            raise zlib.error("the member at %d does not end" % at)
        at = len(data) - len(d.unused_data)
        total += len(t)
        texts.append(t); in_off.append(at); text_off.append(total)
    return b"".join(texts), in_off, text_off


def short_block_member(seed, n_bytes):
    text = far_matches(seed, n_bytes)
    return text, gz(text, level=9, flushes=[(p, zlib.Z_BLOCK) for p in range(3000, len(text), 3000)])


def member_inside_stored_block():
    """a whole gzip member (header, blocks, trailer) as the DATA of a stored block: its header start and its block starts pass
    every test, and no chain lands on them; a second member behind, so that the file has a real boundary too"""
    t1, t2, t3, t4 = fastq(141, 300000), fastq(142, 90000), fastq(143, 200000), fasta(144, 100000)
    inner = gz(t2, flushes=[(p, zlib.Z_BLOCK) for p in range(9000, len(t2), 9000)])
    assert 8000 < len(inner) < 60000
    bw = bgzf_sets.Bits()
    bgzf_sets.stored_block(bw, inner)
    text = t1 + inner + t3
    return wrap(raw(t1, final=False, mem=8) + bw.bytes() + raw(t3, mem=8), text) + gz(t4), inner


def regular():
    """name -> file bytes: all of them inflated exactly at every chunk size"""
    out = {}
    out["three_big_members"] = gz(fastq(101, 900000), level=6) + gz(fasta(102, 700000), level=9) + gz(fastq(103, 600000), level=1)
    many = fastq(104, 120 * 20000)
    out["many_single_block_members"] = b"".join(gz(many[k * 20000:(k + 1) * 20000]) for k in range(120))
    out["empty_members_everywhere"] = EMPTY + gz(fastq(105, 150000)) + EMPTY + EMPTY + gz(fasta(106, 150000), level=9) + gz(fastq(107, 100000), level=1) + EMPTY
    out["one_member"] = gz(fasta(12, 2400000)[:1200000], level=9)      # (gzip_sets.regular()["fasta_level_9"])
    t2, t3 = fastq(108, 200000), fasta(109, 150000)
    out["inner_headers_all_four"] = (gz(fastq(110, 250000))
                                     + wrap(raw(t2), t2, extra=b"AB\x02\x00zz" + b"CD\x00\x00", name=b"x" * 300, comment=b"made by hand", hcrc=True)
                                     + wrap(raw(t3, level=9), t3, extra=b"XY\x05\x00hello", name=b"n" * 300, comment=b"c" * 5000, hcrc=True))
    out["boundary_in_short_blocks"] = short_block_member(111, 350000)[1] + short_block_member(112, 350000)[1]
    out["member_inside_stored_block"] = member_inside_stored_block()[0]
    out["bgzf_as_plain"] = bgzf_sets.bgzf(fastq(113, 150000), block=30011)
    return out


def fastx_members():
    """three_big_members-style files whose text as a whole is one regular FASTQ: (file, text) with the first member ending on a
    record boundary, and with it ending in the middle of a quality line"""
    text = fastq(121, 1500000)
    a = text.index(b"\n@run7.", 600000) + 1
    q = text.index(b"\n+\n", a + 400000) + 3 + 40              # 40 bytes into a quality line
    assert text[a:a + 6] == b"@run7." and b"\n" not in text[q - 40:q + 1]
    return {"record_boundary": (gz(text[:a]) + gz(text[a:a + 500000], level=9) + gz(text[a + 500000:], level=1), text),
            "inside_a_quality_line": (gz(text[:q]) + gz(text[q:], level=1), text)}


# ---- declined files: name -> (bytes, chunk_bytes, reason, gzip member or None) ----
def _base():
    return [gz(fastq(131, 200000)), gz(fasta(132, 150000), level=9), gz(fastq(133, 100000), level=1)]


def distance_over_the_boundary():
    """a good member, then a hand-made one: block 1 n1 literals; block 2 100 literals, a match of 258 bytes at distance 5 000 (in
    front of its member: 100 + n1 < 5 000), literals; two more blocks of literals.  n1 is chosen so that at a chunk of 4096 bytes a
    nominal chunk edge lies between the first bytes of blocks 1 and 2: block 2's start is then the first start of its chunk, a
    chain element begins there, and the match is a marker that narrowing has to refuse through m0.  At a chunk of 65 536 bytes the
    file is one chunk and the run that passed the boundary meets the match itself."""
    first = gz(fastq(134, 200000))
    rng = np.random.RandomState(135)
    lit = [8] * 254 + [9, 9, 9] + [0] * 28 + [9]
    dist = bgzf_sets.lens_of(30, {24: 1, 25: 1})
    letters = np.frombuffer(b"ACGTN", np.uint8)
    for n1 in range(2000, 4800, 100):
        bw = bgzf_sets.Bits()
        bgzf_sets.dynamic_block(bw, lit, dist, [("lit", int(b)) for b in letters[rng.randint(0, 5, n1)]], final=False)
        at2 = len(bw.out)                                   # block 2's first bits are in this byte of the member's deflate data
        bgzf_sets.dynamic_block(bw, lit, dist, [("lit", int(b)) for b in letters[rng.randint(0, 5, 100)]] + [("match", 258, 5000)]
                                + [("lit", int(b)) for b in letters[rng.randint(0, 5, 2800)]], final=False)
        for last in (False, True):
            bgzf_sets.dynamic_block(bw, lit, dist, [("lit", int(b)) for b in letters[rng.randint(0, 5, 3000)]], final=last)
        data = first + wrap(bw.bytes(), b"")                # (trailer: CRC-32 and ISIZE of nothing; no decoder gets that far)
        dn = len(data) - 8 - 10
        nc = max(1, dn // 4096)
        b1, b2 = len(first), len(first) + at2                # the region's bytes (file byte - 10) that hold the first bits of blocks 1 and 2
        if any(b1 < dn * k // nc <= b2 for k in range(1, nc)):
            return data
    raise AssertionError("no n1 puts a chunk edge between the two blocks")


def declined():
    out = {}
    a, b, c = _base()
    good = a + b + c
    offs = [0, len(a), len(a) + len(b)]
    out["trailing_zero_byte"] = (good + b"\x00", 4096, TRAILING, None)
    out["trailing_17_bytes_of_a_header"] = (good + wrap(raw(b"ACGT" * 10), b"ACGT" * 10, name=b"reads.fq")[:17], 4096, TRAILING, None)
    out["inner_method_7"] = (a + b[:2] + b"\x07" + b[3:] + c, 4096, NOT_GZIP, None)
    out["inner_reserved_flag"] = (a + b[:3] + b"\x20" + b[4:] + c, 4096, NOT_GZIP, None)
    t = fastq(136, 60000)
    h = wrap(raw(t), t, name=b"second.fq", hcrc=True)
    bad = bytearray(h); bad[10 + len(b"second.fq") + 1] ^= 0x01
    out["inner_header_crc_wrong"] = (a + bytes(bad) + c, 4096, NOT_GZIP, None)
    out["inner_member_cut_inside_its_data"] = (a + b[:len(b) // 2], 4096, INPUT_END, None)
    members = [a, b, c]
    for m, (delta, reason) in enumerate([(1, OUTPUT_SHORT), (-1, OUTPUT_LONG), (1, OUTPUT_SHORT)]):
        isz = struct.unpack_from("<I", members[m], len(members[m]) - 4)[0]
        parts = list(members)
        parts[m] = members[m][:-4] + struct.pack("<I", isz + delta)
        out["isize_of_member_%d_off_by_one" % m] = (b"".join(parts), 4096, reason, m)
        parts = list(members)
        x = bytearray(members[m]); x[-7] ^= 0x40
        parts[m] = bytes(x)
        out["crc_byte_of_member_%d" % m] = (b"".join(parts), 4096, CRC, m)
    # links must match how a run arrives.  A block start where a header should stand: a member, then raw deflate that begins with
    # a block every test takes, then the trailer of that second text — no magic at H (13).  And a member's start in the middle of
    # a member: behind a stored block, byte-aligned, a whole gzip member without its trailer, then a trailer over both texts — for
    # zlib the 1F behind the stored block is BFINAL 1 / BTYPE 3 (1)
    t1, t2 = fastq(137, 30000), fastq(138, 25000)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    bare = co.compress(t2[:12000]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(t2[12000:]) + co.flush()
    out["block_start_where_a_header_should_be"] = (gz(t1) + bare + struct.pack("<II", zlib.crc32(t2) & 0xFFFFFFFF, len(t2)), 4096, TRAILING, None)
    lead = fastq(139, 6000)[:6000]
    bw = bgzf_sets.Bits()
    bgzf_sets.stored_block(bw, lead)
    inner = gz(t2, flushes=[(12000, zlib.Z_FULL_FLUSH)])
    whole = lead + t2
    out["member_start_in_the_middle_of_a_member"] = (wrap(bw.bytes() + inner[:-8], whole), 4096, BLOCK_TYPE, None)
    far = distance_over_the_boundary()
    out["distance_over_the_boundary_in_a_run"] = (far, 65536, MARKER, None)
    out["distance_over_the_boundary_in_narrowing"] = (far, 4096, MARKER, None)
    return out, offs


def flip_file():
    """three members of about 40 KB of text each, a Z_BLOCK flush every 12 000 text bytes: at a chunk of 4096 bytes every chunk
    has a start and a flip anywhere meets a chunk of the chain"""
    parts = []
    for seed, level in ((151, 6), (152, 9), (153, 1)):
        text = fastq(seed, 40000) if level != 9 else fasta(seed, 40000)
        parts.append(gz(text, level=level, flushes=[(p, zlib.Z_BLOCK) for p in range(12000, len(text), 12000)]))
    return b"".join(parts)


def bit_flips(n=400, seed=177):
    """n copies of flip_file() with one bit flipped each, spread over the whole file (headers and trailers included)"""
    good = flip_file()
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        at = (i * len(good)) // n + int(rng.randint(0, max(len(good) // n, 1)))
        b = bytearray(good); b[min(at, len(good) - 1)] ^= 1 << int(rng.randint(0, 8))
        out.append(bytes(b))
    return out
