"""BGZF files for the inflate tests (tests/test_bgzf_host.py, tests/test_gpu_bgzf.py): members made by zlib's raw deflate and
wrapped in the BGZF header ('BC' subfield with BSIZE) and trailer (CRC-32, ISIZE), hand-made deflate streams that zlib does not
emit (a small bit writer), and damaged files with the member and reason a decoder must report.  Everything is seeded and sized
for seconds; the largest file has a few hundred members."""
import gzip
import random
import struct
import zlib

# reasons (crass_amd/csrc/inflate_core.h)
OK, BLOCK_TYPE, STORED_LEN, CODE_LENGTHS, BAD_SYMBOL, DISTANCE, INPUT_END, OUTPUT_LONG, OUTPUT_SHORT, CRC, NOT_BGZF = range(11)


# ---- members ----
def wrap(deflate, crc, isize, before=b"", after=b"", flags=4, tail=b""):
    """one BGZF member around raw deflate data; before / after: further extra subfields around 'BC'; tail: what the flags announce
    behind the extra field (a file name, a comment)"""
    extra_len = len(before) + 6 + len(after)
    bsize = 12 + extra_len + len(tail) + len(deflate) + 8 - 1
    assert bsize < 65536, bsize
    return (b"\x1f\x8b\x08" + bytes([flags]) + b"\x00\x00\x00\x00\x00\xff" + struct.pack("<H", extra_len) + before + b"BC\x02\x00" +
            struct.pack("<H", bsize) + after + tail + deflate + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """raw deflate of text; flushes: (position, mode) pairs — the compressor is flushed with that mode after text[:position]"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for pos, mode in flushes:
        out += co.compress(text[at:pos]) + co.flush(mode)
        at = pos
    return out + co.compress(text[at:]) + co.flush()


def member(text, **kw):
    wrap_kw = {k: kw.pop(k) for k in ("before", "after", "flags", "tail") if k in kw}
    return wrap(deflate(text, **kw), zlib.crc32(text), len(text), **wrap_kw)


EOF = wrap(b"\x03\x00", 0, 0)
assert len(EOF) == 28


def bgzf(text, block=60000, eof=True, **kw):
    return b"".join(member(text[i:i + block], **kw) for i in range(0, len(text), block)) + (EOF if eof else b"")


def walk(data):
    """the header walk restated (what crass_bgzf_index_host must give): (in_off, out_off, data_off), or None with the position and
    index of the member that does not parse.  It is bgzf_walk (host_inflate.cpp) plus the one thing the index adds: the start of the
    deflate data behind a file name, a comment and a header CRC where the flags announce them — a member in which those run into
    the trailer is declined here and accepted by bgzf_walk, which never looks at them (not_bgzf: file_name_runs_into_the_trailer)"""
    ioff, ooff, doff, p, o = [], [], [], 0, 0
    if not data:
        return None, 0, 0
    while p < len(data):
        bad = (None, p, len(ioff))
        if len(data) - p < 28 or data[p:p + 3] != b"\x1f\x8b\x08" or not data[p + 3] & 4:
            return bad
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        if p + 12 + xlen > len(data):
            return bad
        total, q = 0, p + 12
        while q + 4 <= p + 12 + xlen:
            slen = struct.unpack_from("<H", data, q + 2)[0]
            if data[q:q + 2] == b"BC" and slen == 2 and q + 6 <= p + 12 + xlen:
                total = struct.unpack_from("<H", data, q + 4)[0] + 1
            q += 4 + slen
        if total < 12 + xlen + 10 or p + total > len(data):
            return bad
        isz = struct.unpack_from("<I", data, p + total - 4)[0]
        if isz > 65536:
            return bad
        d, end = p + 12 + xlen, p + total - 8
        for bit in (8, 16):
            if data[p + 3] & bit:
                while d < end and data[d]:
                    d += 1
                if d >= end:
                    return bad
                d += 1
        if data[p + 3] & 2:
            d += 2
        if d > end:
            return bad
        ioff.append(p); ooff.append(o); doff.append(d)
        p += total; o += isz
    return (ioff + [p], ooff + [o], doff), 0, 0


def zlib_members(data):
    """zlib's view of an accepted file: per member (text, ok) — ok False where zlib raises, stops before the final block's end, or
    its text disagrees with the trailer's ISIZE or CRC-32"""
    (ioff, ooff, doff), _, _ = walk(data)
    out = []
    for m in range(len(doff)):
        raw, end = data[doff[m]:ioff[m + 1] - 8], ioff[m + 1] - 8
        crc, isz = struct.unpack_from("<II", data, end)
        try:
            d = zlib.decompressobj(-15)
            text = d.decompress(raw, 65536 + 1024)
            ok = d.eof and len(text) == isz and zlib.crc32(text) == crc
        except zlib.error:
            text, ok = b"", False
        out.append((text, ok))
    return out


# ---- a bit writer and hand-made deflate blocks ----
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, k):
        """k bits of value, lowest first"""
        self.acc |= (value & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, k):
        """a Huffman code of k bits, highest first (RFC 1951 3.1.1)"""
        for i in range(k - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2), whatever its Kraft sum"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6          # a complete code-length code in which every symbol has a code


def len_symbol(n, force=None):
    s = force if force is not None else max(i for i in range(29) if LEN_BASE[i] <= n and (i == 28 or n < LEN_BASE[i] + (1 << LEN_EXTRA[i])))
    return 257 + s, n - LEN_BASE[s], LEN_EXTRA[s]


def dist_symbol(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, d - DIST_BASE[s], DIST_EXTRA[s]


def apply_tokens(tokens, text=b""):
    out = bytearray(text)
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


def dynamic_block(bw, lit_lens, dist_lens, tokens, final=True, cl_syms=None, end=True):
    """a dynamic block: the code lengths as given (nothing checks them), sent one by one or as the code-length symbols cl_syms
    ((symbol, extra value) pairs); then the tokens ('lit', byte) / ('match', length, distance) and the end-of-block code"""
    bw.put(1 if final else 0, 1); bw.put(2, 2)
    bw.put(len(lit_lens) - 257, 5); bw.put(len(dist_lens) - 1, 5); bw.put(19 - 4, 4)
    for s in CL_ORDER:
        bw.put(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    if cl_syms is None:
        cl_syms = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    for s, extra in cl_syms:
        bw.code(*cl[s])
        if s >= 16:
            bw.put(extra, {16: 2, 17: 3, 18: 7}[s])
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if t[0] == "lit":
            bw.code(*lit[t[1]])
        else:
            s, ev, eb = len_symbol(t[1], t[3] if len(t) > 3 else None)
            bw.code(*lit[s]); bw.put(ev, eb)
            s, ev, eb = dist_symbol(t[2])
            bw.code(*dist[s]); bw.put(ev, eb)
    if end:
        bw.code(*lit[256])


def stored_block(bw, data, final=False, nlen=None):
    bw.put(1 if final else 0, 1); bw.put(0, 2); bw.align()
    bw.put(len(data), 16); bw.put((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    bw.out += data


def lens_of(n, assign):
    lens = [0] * n
    for s, l in assign.items():
        lens[s] = l
    return lens


def hand_made():
    """name -> (deflate data, text): streams zlib accepts but does not write"""
    out = {}
    A, Cc, G, T, NL = 65, 67, 71, 84, 10
    # a literal / length code with a 15-bit codeword (lengths 1 .. 15, 15); no distance code used
    assign = {A: 1, Cc: 2, G: 3, T: 4, NL: 5, 256: 6}
    assign.update({48 + k: 7 + k for k in range(9)}); assign[57] = 15
    toks = [("lit", b) for b in (A, 56, Cc, 57, G, T, NL, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, A, A)]
    bw = Bits(); dynamic_block(bw, lens_of(257, assign), [0], toks)
    out["codeword_15_bits"] = (bw.bytes(), apply_tokens(toks))
    # a single distance code of one bit
    toks = [("lit", A), ("match", 3, 1), ("lit", A), ("match", 4, 1)]
    bw = Bits(); dynamic_block(bw, lens_of(259, {A: 1, 256: 2, 257: 3, 258: 3}), [1], toks)
    out["one_distance_code_of_one_bit"] = (bw.bytes(), apply_tokens(toks))
    # no distance code used
    toks = [("lit", b) for b in b"ACCA\nAC"]
    bw = Bits(); dynamic_block(bw, lens_of(257, {A: 1, Cc: 2, NL: 3, 256: 3}), [0], toks)
    out["no_distance_code"] = (bw.bytes(), apply_tokens(toks))
    # repeat code 16 that runs from the literal lengths into the distance lengths
    lit = lens_of(260, {A: 2, Cc: 2, 256: 3, 257: 3, 258: 3, 259: 3})
    dist = [3, 3, 3, 3, 2, 2]
    cl = [(18, 65 - 11), (2, 0), (0, 0), (2, 0), (18, 138 - 11), (18, 50 - 11), (3, 0), (16, 6 - 3), (3, 0), (2, 0), (2, 0)]
    toks = [("lit", A), ("lit", Cc), ("lit", A), ("lit", A), ("lit", Cc), ("lit", Cc), ("lit", A), ("match", 4, 2), ("match", 5, 6), ("match", 5, 3), ("match", 3, 5)]
    bw = Bits(); dynamic_block(bw, lit, dist, toks, cl_syms=cl)
    out["repeat_16_across_the_edge"] = (bw.bytes(), apply_tokens(toks))
    # repeat codes 17 and 18 (zeros) doing the same
    for name, hlit, nz in (("repeat_17_across_the_edge", 262, 6), ("repeat_18_across_the_edge", 266, 14)):
        lit = lens_of(hlit, {A: 1, 256: 2, 257: 2})
        dist = [0] * 6 + [1, 1]
        sym = (17, nz - 3) if nz <= 10 else (18, nz - 11)
        cl = [(18, 65 - 11), (1, 0), (18, 138 - 11), (18, 52 - 11), (2, 0), (2, 0), sym] + ([(17, 4 - 3)] if nz == 6 else []) + [(1, 0), (1, 0)]
        toks = [("lit", A)] * 14 + [("match", 3, 9), ("match", 3, 12), ("match", 3, 13), ("match", 3, 16)]
        bw = Bits(); dynamic_block(bw, lit, dist, toks, cl_syms=cl)
        out[name] = (bw.bytes(), apply_tokens(toks))
    # length symbol 285 (258 bytes, no extra bits)
    toks = [("lit", A), ("match", 258, 1), ("lit", A)]
    bw = Bits(); dynamic_block(bw, lens_of(286, {A: 1, 256: 2, 285: 2}), [1, 1], toks)
    out["length_symbol_285"] = (bw.bytes(), apply_tokens(toks))
    # distance symbols 28 and 29 with their 13 extra bits, behind a stored block of 30 000 bytes
    rng = random.Random(28)
    front = bytes(rng.randrange(256) for _ in range(30000))
    toks = [("match", 3, 16385), ("match", 3, 16385 + 8191), ("match", 3, 24577), ("match", 3, 24577 + 5000), ("lit", A), ("match", 258, 30000)]
    bw = Bits(); stored_block(bw, front)
    dynamic_block(bw, lens_of(286, {A: 1, 256: 2, 257: 3, 285: 3}), lens_of(30, {28: 1, 29: 1}), toks)
    out["distance_symbols_28_29"] = (bw.bytes(), apply_tokens(toks, front))
    # a match at the full distance of 32 768 (zlib's own matches stop 262 short of it)
    front = bytes(rng.randrange(256) for _ in range(32768))
    toks = [("match", 258, 32768), ("match", 3, 32768), ("lit", A), ("match", 258, 32768)]
    bw = Bits(); stored_block(bw, front)
    dynamic_block(bw, lens_of(286, {A: 1, 256: 2, 257: 3, 285: 3}), lens_of(30, {28: 1, 29: 1}), toks)
    out["distance_32768"] = (bw.bytes(), apply_tokens(toks, front))
    return out


def hand_made_members():
    """name -> (member bytes, text)"""
    return {k: (wrap(d, zlib.crc32(t), len(t)), t) for k, (d, t) in hand_made().items()}


# ---- texts ----
def fastq(rng, n, name=b"r"):
    recs = []
    for i in range(n):
        s = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(30, 150)))
        recs.append(b"@%s%d lane=%d\n%s\n+\n%s\n" % (name, i, i % 4, s, bytes(rng.choice(b"FFFFF:,#") for _ in s)))
    return recs


def regular():
    """name -> BGZF file bytes, all of them inflated exactly"""
    rng = random.Random(14)
    out = {}
    out["eof_alone"] = EOF
    out["one_byte"] = member(b"A") + EOF
    noise = bytes(rng.choice(b"ACGTN\n") for _ in range(65536))
    out["text_65536"] = member(noise) + EOF
    out["text_65280"] = member(noise[:65280], level=1) + EOF
    rnd = bytes(rng.randrange(256) for _ in range(9000))
    out["stored_level_0"] = member(rnd, level=0) + EOF
    out["stored_empty_sync_flush"] = member(rnd[:3000], level=0, flushes=((1000, zlib.Z_SYNC_FLUSH), (1000, zlib.Z_SYNC_FLUSH))) + EOF
    # a stored block that starts off a byte boundary: a fixed block in front of it leaves the bit position inside a byte
    bw = Bits()
    bw.put(0, 1); bw.put(1, 2)                            # fixed block: 'A' (0x30 + 65, 8 bits), end-of-block (7 zero bits)
    bw.code(0x30 + 65, 8); bw.code(0, 7)
    assert bw.n != 0
    stored_block(bw, rnd[:777], final=True)
    out["stored_off_a_byte_edge"] = wrap(bw.bytes(), zlib.crc32(b"A" + rnd[:777]), 778) + EOF
    out["fixed_huffman"] = member(noise[:5000], strategy=zlib.Z_FIXED) + member(b"ACGTACGTAC" * 30, strategy=zlib.Z_FIXED) + EOF
    reps = b"".join(fastq(rng, 300))
    half = len(reps) // 2
    cross = reps[:half] + reps[half - 200:half - 100] + reps[half:]      # a match that reaches back across the block edge
    out["several_dynamic_blocks"] = member(cross[:60000], flushes=((half, zlib.Z_FULL_FLUSH),)) + member(cross[:60000], flushes=((half, zlib.Z_SYNC_FLUSH), (half + 5000, zlib.Z_BLOCK))) + EOF
    out["run_distance_1"] = member(b"A" * 60000) + EOF
    out["run_distance_2_3"] = member(b"AC" * 30000 + b"A") + member(b"ACG" * 20000 + b"AC") + member((b"ACG" * 9 + b"T") * 2000) + EOF
    p37, p64, p100 = bytes(rng.choice(b"ACGT") for _ in range(37)), bytes(rng.choice(b"ACGT") for _ in range(64)), bytes(rng.choice(b"ACGT") for _ in range(100))
    out["overlap_below_and_above_64"] = member(p37 * 1500) + member(p64 * 900 + p64[:13]) + member(p100 * 600) + member(bytes(rng.randrange(256) for _ in range(63)) * 1000) + EOF
    blk = bytes(rng.randrange(256) for _ in range(32400))
    out["distance_near_the_window"] = member(blk + blk[:300] + blk[5:900], level=9) + EOF
    seed = bytes(rng.randrange(256) for _ in range(40))
    out["distance_equals_produced"] = member(seed + seed + seed[:7], level=9) + member(b"AB" + b"AB" * 40, level=9) + EOF
    fa = b""
    for i in range(400):
        sq = bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(1, 400)))
        fa += b">s%d some words\r\n%s\r\n" % (i, b"\r\n".join(sq[k:k + 60] for k in range(0, len(sq), 60)))
    out["fasta_wrapped_crlf"] = bgzf(fa, block=20011)
    # four-line FASTQ whose records, lines and the '@' itself fall on member edges
    recs = fastq(rng, 900)
    text = b"".join(recs)
    cuts, at = [0], 0
    for i, r in enumerate(recs[:-1]):
        at += len(r)
        if i % 90 == 10:
            cuts.append(at)                               # between two records: the next member starts with '@'
        elif i % 90 == 40:
            cuts.append(at + 1)                           # ... right behind that '@'
        elif i % 90 == 70:
            cuts.append(at + r.index(b"\n") + 1 - len(r))     # behind the record's header line
    cuts = sorted(set(cuts)) + [len(text)]
    out["fastq_edges_on_members"] = b"".join(member(text[a:b]) for a, b in zip(cuts, cuts[1:])) + EOF
    small = fastq(rng, 2100, b"m")
    grouped = lambda n: b"".join(member(b"".join(small[3 * i:3 * i + 3])) for i in range(n))
    for n in (1, 63, 64, 65):
        out["members_%d" % n] = grouped(n)
    out["members_700"] = grouped(700) + EOF             # more members than one launch has waves
    part = lambda a, b: b"".join(recs[a:b])
    out["empty_members_in_the_middle"] = member(part(0, 20)) + EOF + member(b"") + member(part(20, 40)) + EOF + EOF + member(part(40, 60))
    out["subfields_around_BC"] = (member(part(0, 15), before=b"XY\x03\x00abc", after=b"ZZ\x00\x00") + member(part(15, 30), after=b"BC\x01\x00q") +
                                  member(part(30, 35), flags=4 | 8 | 16, tail=b"name.fq\x00a comment\x00") + EOF)
    for k, (m, t) in hand_made_members().items():
        out["hand_" + k] = member(text[:1000]) + m + member(text[1000:1500]) + EOF
    return out


def fastx_regular():
    """the regular files whose text is a regular FASTA / FASTQ"""
    return ["fasta_wrapped_crlf", "fastq_edges_on_members", "members_1", "members_63", "members_64", "members_65", "members_700",
            "empty_members_in_the_middle", "subfields_around_BC"]


# ---- damaged files: name -> (bytes, member, reason) ----
def _members(n=5, seed=3):
    rng = random.Random(seed)
    return [member(b"".join(fastq(rng, 60, b"d%d_" % k))) for k in range(n)]


def _raw_member(bw, isize=10, crc=0):
    return wrap(bw.bytes(), crc, isize)


def damaged():
    out = {}
    ms = _members()
    def put(name, k, bad, reason):
        out[name] = (b"".join(ms[:k]) + bad + b"".join(ms[k + 1:]) + EOF, k, reason)
    def poke(m, at, f):
        b = bytearray(m); b[at] = f(b[at]); return bytes(b)
    put("crc_byte_flipped", 2, poke(ms[2], len(ms[2]) - 7, lambda x: x ^ 0x40), CRC)
    isz = struct.unpack_from("<I", ms[1], len(ms[1]) - 4)[0]
    put("isize_one_more", 1, ms[1][:-4] + struct.pack("<I", isz + 1), OUTPUT_SHORT)
    put("isize_one_less", 1, ms[1][:-4] + struct.pack("<I", isz - 1), OUTPUT_LONG)
    bw = Bits(); bw.put(1, 1); bw.put(3, 2); bw.put(0, 13)
    put("block_type_3", 3, _raw_member(bw), BLOCK_TYPE)
    bw = Bits(); stored_block(bw, b"0123456789", final=True, nlen=(~10 & 0xFFFF) ^ 0x0100)
    put("stored_len_nlen", 0, _raw_member(bw), STORED_LEN)
    A = 65
    bw = Bits(); dynamic_block(bw, lens_of(257, {A: 1, 66: 1, 256: 1}), [0], [])
    put("code_over_subscribed", 4, _raw_member(bw), CODE_LENGTHS)
    bw = Bits(); dynamic_block(bw, lens_of(257, {A: 2, 66: 2, 256: 2}), [0], [("lit", A)])
    put("code_incomplete", 2, _raw_member(bw), CODE_LENGTHS)
    bw = Bits(); dynamic_block(bw, lens_of(257, {A: 1, 256: 1}), [2, 2, 2], [("lit", A)])
    put("distance_code_incomplete", 2, _raw_member(bw), CODE_LENGTHS)
    bw = Bits(); dynamic_block(bw, lens_of(257, {A: 1, 256: 1}), [0], [("lit", A)], cl_syms=[(16, 0)] + [(0, 0)] * 62 + [(1, 0)] + [(18, 127)] + [(18, 52 - 11)] + [(1, 0), (0, 0)])
    put("repeat_16_first", 1, _raw_member(bw), CODE_LENGTHS)
    bw = Bits(); dynamic_block(bw, lens_of(257, {A: 1, 256: 1}), [0], [("lit", A)], cl_syms=[(18, 65 - 11), (1, 0), (18, 138 - 11), (18, 138 - 11)])
    put("repeat_past_the_end", 1, _raw_member(bw), CODE_LENGTHS)
    bw = Bits(); dynamic_block(bw, lens_of(257, {A: 1, 66: 1}), [0], [("lit", A)] * 10, end=False)
    put("no_end_of_block_code", 3, _raw_member(bw), CODE_LENGTHS)
    t = b"".join(fastq(random.Random(8), 60))
    put("deflate_data_cut_short", 2, wrap(deflate(t)[:-5], zlib.crc32(t), len(t)), INPUT_END)
    bw = Bits(); dynamic_block(bw, lens_of(258, {A: 1, 256: 2, 257: 2}), [0, 0, 1], [("lit", A), ("lit", A), ("match", 3, 3)])
    put("distance_one_beyond", 0, _raw_member(bw), DISTANCE)
    bw = Bits(); dynamic_block(bw, lens_of(258, {A: 1, 256: 2, 257: 2}), [1], [("lit", A)], end=False)
    bw.code(*canonical(lens_of(258, {A: 1, 256: 2, 257: 2}))[257]); bw.put(1, 1); bw.put(0, 16)      # length 3, then the bit that is no distance code
    put("bit_pattern_that_is_no_code", 0, _raw_member(bw), BAD_SYMBOL)
    bw = Bits(); bw.put(1, 1); bw.put(1, 2); bw.code(0xC6, 8)          # fixed block, length symbol 286
    put("length_symbol_286", 4, _raw_member(bw), BAD_SYMBOL)
    bw = Bits(); bw.put(1, 1); bw.put(1, 2); bw.code(0x30 + A, 8); bw.code(1, 7); bw.code(30, 5)      # ... 'A', length 3, distance symbol 30
    put("distance_symbol_30", 4, _raw_member(bw), BAD_SYMBOL)
    bad1 = poke(ms[1], len(ms[1]) - 6, lambda x: x ^ 1)
    bw = Bits(); bw.put(1, 1); bw.put(3, 2); bw.put(0, 13)
    out["two_damaged_members"] = (ms[0] + bad1 + ms[2] + _raw_member(bw) + ms[4] + EOF, 1, CRC)
    return out


def not_bgzf():
    """name -> (bytes, member, position)"""
    ms = _members(3)
    text = b"".join(fastq(random.Random(5), 50))
    return {
        "plain_gzip": (gzip.compress(text), 0, 0),
        "empty_file": (b"", 0, 0),
        "plain_gzip_behind_members": (ms[0] + ms[1] + gzip.compress(text), 2, len(ms[0]) + len(ms[1])),
        "cut_inside_a_member": (ms[0] + ms[1][:-3], 1, len(ms[0])),
        "no_BC_subfield": (ms[0] + wrap(deflate(text), zlib.crc32(text), len(text)).replace(b"BC\x02\x00", b"BD\x02\x00", 1), 1, len(ms[0])),
        "isize_beyond_64k": (ms[0][:-4] + struct.pack("<I", 65537), 0, 0),
        "short_tail": (ms[0] + EOF[:27], 1, len(ms[0])),
        "file_name_runs_into_the_trailer": (ms[0] + wrap(b"\x07\x07\x07", 0, 0, flags=4 | 8), 1, len(ms[0])),
    }


def bit_flips(n=200, seed=77):
    """[(file bytes, member that was hit)]: one bit flipped inside the deflate data of one member of a five-member file"""
    ms = _members(5, seed=9)
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = rng.randrange(5)
        at = rng.randrange(18, len(ms[k]) - 8)
        b = bytearray(ms[k]); b[at] ^= 1 << rng.randrange(8)
        out.append((b"".join(ms[:k]) + bytes(b) + b"".join(ms[k + 1:]) + EOF, k))
    return out
