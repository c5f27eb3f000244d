"""Plain (single-member) gzip files for the gunzip tests (tests/test_gzip_host.py, tests/test_gpu_gzip.py): texts compressed with
zlib.compressobj(level, DEFLATED, 31, 9, strategy) or as raw deflate behind hand-built headers, and damaged files with the reason a
decoder must report.  A few hundred KB to about 1 MB of compressed bytes per file: the smallest shapes at which the chunk rule
(crass_amd/csrc/gunzip_core.h) can go wrong — at a chunk of 4096 bytes that is tens to hundreds of chunks.  Everything is seeded."""
import struct
import zlib

import numpy as np

from tests import bgzf_sets

# reasons (crass_amd/csrc/inflate_core.h)
OK, BLOCK_TYPE, STORED_LEN, CODE_LENGTHS, BAD_SYMBOL, DISTANCE, INPUT_END, OUTPUT_LONG, OUTPUT_SHORT, CRC, NOT_BGZF, NOT_GZIP, NO_START, TRAILING, MARKER = range(15)
CHUNKS = (4096, 16384, 65536, 0)
FLIP_CHUNK = 4096


def gz(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """text as one gzip member; flushes: (position, mode) pairs — the compressor is flushed with that mode after text[:position]"""
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    out, at = [], 0
    for pos, mode in flushes:
        out.append(co.compress(text[at:pos]) + co.flush(mode))
        at = pos
    return b"".join(out) + co.compress(text[at:]) + co.flush()


def wrap(deflate, text, extra=None, name=None, comment=None, hcrc=False):
    """a hand-built gzip member around raw deflate data: FEXTRA / FNAME / FCOMMENT / FHCRC as asked"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\xff"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + deflate + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF)


def raw(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, final=True, mem=9):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return co.compress(text) + (co.flush() if final else co.flush(zlib.Z_FULL_FLUSH))


# ---- texts ----
def fastq(seed, n_bytes):
    """four-line FASTQ of about n_bytes: reads of 100 .. 150 bases, qualities that mostly repeat"""
    rng = np.random.RandomState(seed)
    recs, size, i = [], 0, 0
    while size < n_bytes:
        L = int(rng.randint(100, 151))
        s = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, L)].tobytes()
        q = np.frombuffer(b"FFFFFFFF:,#F", np.uint8)[rng.randint(0, 12, L)].tobytes()
        r = b"@run7.%d lane=%d/1\n%s\n+\n%s\n" % (i, i % 4, s, q)
        recs.append(r); size += len(r); i += 1
    return b"".join(recs)


def fasta(seed, n_bytes):
    """FASTA wrapped at 60 columns, sequences of 200 .. 3000 bases"""
    rng = np.random.RandomState(seed)
    recs, size, i = [], 0, 0
    while size < n_bytes:
        L = int(rng.randint(200, 3001))
        s = np.frombuffer(b"ACGTN", np.uint8)[rng.randint(0, 5, L)].tobytes()
        r = b">contig_%d len=%d\n%s\n" % (i, L, b"\n".join(s[k:k + 60] for k in range(0, L, 60)))
        recs.append(r); size += len(r); i += 1
    return b"".join(recs)


def far_matches(seed, n_bytes):
    """text over 16 letters in which every 3 000 bytes hold copies of what stood 20 .. 32 KB in front"""
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGTNacgtnRYKMSW", np.uint8)
    out = bytearray(letters[rng.randint(0, 16, 33000)].tobytes())
    while len(out) < n_bytes:
        out += letters[rng.randint(0, 16, 2200)].tobytes()
        for _ in range(2):
            back = int(rng.randint(20000, 32600))
            n = int(rng.randint(100, 400))
            at = len(out) - back
            out += out[at:at + n]
    return bytes(out)


def short_blocks():
    """a Z_BLOCK flush every ~3 000 text bytes over far_matches: blocks of about 1.5 KB, so at a chunk of 4096 bytes every chunk
    has a start, consecutive chain chunks are each shorter than the window, and a window shows text from two and three chunks back"""
    text = far_matches(31, 700000)
    return text, gz(text, level=9, flushes=[(p, zlib.Z_BLOCK) for p in range(3000, len(text), 3000)])


def distance_32768():
    """a 32 768-byte random block, then nothing but matches of 258 bytes at distance exactly 32 768 (zlib's own matches stop 262
    short of that, so the stream is made by hand): literal blocks of 4096 bytes, then blocks of 400 matches, each about 1.5 KB of
    input and 100 KB of text, so that the text of a chain chunk is copied from the chunk before it over every chunk edge"""
    rng = np.random.RandomState(21)
    blk = rng.randint(0, 256, 32768).astype(np.uint8).tobytes()
    lit = [8] * 254 + [9, 9, 9] + [0] * 28 + [9]           # literals, end-of-block and length symbol 285: a complete code
    dist = bgzf_sets.lens_of(30, {28: 1, 29: 1})
    bw = bgzf_sets.Bits()
    for at in range(0, 32768, 4096):
        bgzf_sets.dynamic_block(bw, lit, dist, [("lit", b) for b in blk[at:at + 4096]], final=False)
    n_blocks = 40
    for k in range(n_blocks):
        bgzf_sets.dynamic_block(bw, lit, dist, [("match", 258, 32768)] * 400, final=k == n_blocks - 1)
    text = bgzf_sets.apply_tokens([("match", 258 * 400 * n_blocks, 32768)], blk)
    return text, wrap(bw.bytes(), text)


def embedded_stream():
    """ordinary blocks, then stored blocks whose DATA is another deflate stream (block starts that pass every test and that no
    chain ever lands on), then ordinary blocks again"""
    t1, t3 = fastq(41, 400000), fastq(43, 300000)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    t2 = fastq(42, 90000)
    inner = b"".join(co.compress(t2[at:at + 9000]) + co.flush(zlib.Z_BLOCK) for at in range(0, len(t2), 9000)) + co.flush()
    assert 8000 < len(inner) < 60000                      # (far inside the span at a chunk of 4096 bytes)
    bw = bgzf_sets.Bits()
    bgzf_sets.stored_block(bw, inner)                     # (one stored block: its blocks follow each other as in a stream of their own)
    text = t1 + inner + t3
    # (memLevel 8: blocks of about 20 KB, so that the chunk that crosses the stored block — the rest of its own block, 25 KB of
    # stored data whose starts are not for it, and the whole block behind, whose start hides behind a false one in the same
    # chunk — stays far inside the span at a chunk of 4096 bytes)
    return text, wrap(raw(t1, final=False, mem=8) + bw.bytes() + raw(t3, mem=8), text)


def regular():
    """name -> (file bytes, text): all of them inflated exactly at every chunk size"""
    out = {}
    def put(name, text, **kw):
        out[name] = (gz(text, **kw), text)
    put("empty_text", b"")
    put("one_byte", b"A")
    noise = fasta(5, 70000)
    for n in (32767, 32768, 32769, 65536):
        put("text_%d" % n, noise[:n])
    fq, fa = fastq(11, 2600000), fasta(12, 2400000)
    for level in (1, 6, 9):
        put("fastq_level_%d" % level, fq, level=level)
    put("fasta_level_1", fa[:1200000], level=1)
    put("fasta_level_6", fa, level=6)
    put("fasta_level_9", fa[:1200000], level=9)
    put("fastq_huffman_only", fq[:900000], strategy=zlib.Z_HUFFMAN_ONLY)
    put("fasta_huffman_only", fa[:900000], strategy=zlib.Z_HUFFMAN_ONLY)
    put("run_of_A", b"A" * 300000)
    text, data = distance_32768()
    out["random_block_repeated"] = (data, text)
    text, data = short_blocks()
    out["short_blocks"] = (data, text)
    fl = fq[:1500000]
    put("sync_flushes", fl, flushes=[(p, zlib.Z_SYNC_FLUSH) for p in range(50000, len(fl), 70001)])
    put("full_flushes", fl, flushes=[(p, zlib.Z_FULL_FLUSH) for p in range(30000, len(fl), 90001)])
    hd = fq[:300000]
    d = raw(hd)
    out["header_fextra"] = (wrap(d, hd, extra=b"XY\x05\x00hello"), hd)
    out["header_fname"] = (wrap(d, hd, name=b"reads_1.fastq"), hd)
    out["header_fcomment"] = (wrap(d, hd, comment=b"made by hand"), hd)
    out["header_fhcrc"] = (wrap(d, hd, hcrc=True), hd)
    out["header_all_four"] = (wrap(d, hd, extra=b"AB\x02\x00zz" + b"CD\x00\x00", name=b"x" * 300, comment=b"c" * 70000, hcrc=True), hd)
    text, data = embedded_stream()
    out["embedded_stream_in_stored_blocks"] = (data, text)
    return out


def chained():
    """the sets whose chain must really be made of many chunks (tests/test_gzip_host.py pins the chunk size per set)"""
    return ["fastq_level_6", "fasta_level_6", "short_blocks"]


def fastx_regular():
    """the regular files whose text is a regular FASTA / FASTQ and that are more than one chunk at the default chunk size: reads of
    ragged lengths, and in the FASTA one reads with N (exception reads)"""
    return ["fastq_level_6", "fasta_level_6"]


# ---- declined files: name -> (bytes, chunk_bytes, reason) ----
def declined():
    out = {}
    fq = fastq(51, 500000)
    good = gz(fq)
    out["two_members"] = (good + gz(fq[:1000]), 4096, TRAILING)
    out["one_trailing_byte"] = (good + b"\x00", 4096, TRAILING)
    isz = struct.unpack_from("<I", good, len(good) - 4)[0]
    out["isize_one_more"] = (good[:-4] + struct.pack("<I", isz + 1), 4096, OUTPUT_SHORT)
    out["isize_one_less"] = (good[:-4] + struct.pack("<I", isz - 1), 4096, OUTPUT_LONG)
    b = bytearray(good); b[-7] ^= 0x40
    out["crc_byte_flipped"] = (bytes(b), 4096, CRC)
    named = wrap(raw(fq[:5000]), fq[:5000], name=b"n" * 40)
    out["cut_inside_the_header"] = (named[:30], 4096, NOT_GZIP)
    out["cut_before_the_flags"] = (good[:3], 4096, NOT_GZIP)
    # (a cut file's last 8 bytes are taken for its trailer, so the deflate data ends early either way; with at most 32 chunks no
    # run stops at the span's end, so the chain's last chunk is the one that runs into the end of the data)
    small = gz(fq[:200000])
    assert len(small) // 2 < len(small) - 3 < 32 * 4096
    out["cut_inside_the_deflate_data"] = (small[:len(small) // 2], 4096, INPUT_END)
    out["cut_inside_the_trailer"] = (small[:-3], 4096, INPUT_END)
    out["not_deflate"] = (b"\x1f\x8b\x07" + good[3:], 4096, NOT_GZIP)
    out["reserved_flag"] = (good[:3] + b"\x20" + good[4:], 4096, NOT_GZIP)
    out["header_crc_wrong"] = (wrap(raw(fq[:5000]), fq[:5000], hcrc=True)[:10] + b"\x00\x00" + raw(fq[:5000]) + good[-8:], 4096, NOT_GZIP)
    out["block_type_3"] = (wrap(raw(fq[:200000], final=False) + b"\x07\x00", fq[:200000]), 4096, BLOCK_TYPE)
    rnd = np.random.RandomState(52).randint(0, 256, 200000).astype(np.uint8).tobytes()
    out["level_0_beyond_the_span"] = (gz(rnd, level=0), 4096, NO_START)
    out["fixed_beyond_the_span"] = (gz(fq[:450000], strategy=zlib.Z_FIXED), 4096, NO_START)
    return out


def accepted_at_a_larger_chunk():
    """the inputs of reason 12 at a chunk size where they fit: name -> (bytes, chunk_bytes, text)"""
    d = declined()
    rnd = np.random.RandomState(52).randint(0, 256, 200000).astype(np.uint8).tobytes()
    return {"level_0": (d["level_0_beyond_the_span"][0], 65536, rnd), "fixed": (d["fixed_beyond_the_span"][0], 65536, fastq(51, 500000)[:450000])}


def flip_file():
    """the FASTQ file the bit flips are made of: a Z_BLOCK flush every 12 000 text bytes, so that at a chunk of 4096 bytes its
    seven or eight chunks all have starts and a flip anywhere meets a chunk of the chain"""
    text = fastq(61, 120000)
    return gz(text, flushes=[(p, zlib.Z_BLOCK) for p in range(12000, len(text), 12000)])


def bit_flips(n=200, seed=77):
    """n copies of flip_file() with one bit flipped each, spread over the whole file (header and trailer included)"""
    good = flip_file()
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        at = (i * len(good)) // n + int(rng.randint(0, max(len(good) // n, 1)))
        b = bytearray(good); b[min(at, len(good) - 1)] ^= 1 << int(rng.randint(0, 8))
        out.append(bytes(b))
    return out
