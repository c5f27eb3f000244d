"""Sets of several input files for the tests of crass_fastx_files_scan_host / crass_hip_load_fastx_files (tests/test_fastx_files_host.py,
tests/test_gpu_fastx_files.py): every set is a list of files' bytes — plain FASTA / FASTQ and BGZF (tests/bgzf_sets.py makes the
members) — of a few hundred records of 0 .. 300 bases, seeded.  accepted(): name -> files; declined(): name -> (files, verdict) with
verdict = (file, FASTA / FASTQ reason, position in that file, BGZF reason, member) as the host and the device must report it."""
import random

from tests import bgzf_sets

ALPHA = b"ACGT"


def read(rng, n, odd=False):
    """n bases; odd: an N, lower case or a byte 0xFF among them (0xFF is no sequence byte: kseq drops it, the read is n - 1 long)"""
    s = bytearray(rng.choice(ALPHA) for _ in range(n))
    if odd and n:
        k = rng.randrange(n)
        s[k] = rng.choice([ord("N"), ord("a"), ord("g"), 0xFF])
    return bytes(s)


def n_graph(s):
    return sum(1 for b in s if 33 <= b <= 126)


def fasta(names, seqs, eol=b"\n", wrap=0, final_eol=True):
    out = []
    for nm, s in zip(names, seqs):
        body = eol.join(s[k:k + wrap] for k in range(0, len(s), wrap)) if wrap and s else s
        out.append(b">" + nm + eol + body + eol)
    t = b"".join(out)
    return t if final_eol else t[:len(t) - len(eol)]


def fastq(names, seqs, eol=b"\n", final_eol=True, rng=None):
    out = []
    for k, (nm, s) in enumerate(zip(names, seqs)):
        q = bytes((33 + (7 * k + i) % 90) if not rng else rng.randrange(33, 127) for i in range(n_graph(s)))
        q = q.replace(b"@", b"A") if q[:1] == b"@" else q          # (a quality line may start with '@': kept rare, not excluded)
        out.append(b"@" + nm + eol + s + eol + b"+" + eol + q + eol)
    t = b"".join(out)
    return t if final_eol else t[:len(t) - len(eol)]


def names(prefix, n, comment=None):
    return [(b"%s%d" % (prefix, i)) + ((b" " + comment + b"%d" % i) if comment else b"") for i in range(n)]


def lens(rng, n, lo=0, hi=300):
    return [rng.choice([0, 1, 15, 16, 17, 31, 32, 33, 64, 150, 300, rng.randint(lo, hi)]) for _ in range(n)]


def accepted():
    rng = random.Random(1507)
    sets = {}
    sq = lambda n, **kw: [read(rng, l, odd=(i % 9 == 0)) for i, l in enumerate(lens(rng, n, **kw))]
    # FASTA + FASTQ mixed
    sets["fasta_fastq"] = [fasta(names(b"a", 200), sq(200)), fastq(names(b"q", 180, b"c"), sq(180))]
    # plain + BGZF (several members, with the end-of-file member)
    t = fastq(names(b"z", 300, b"lane"), sq(300))
    sets["plain_bgzf"] = [fasta(names(b"p", 150), sq(150)), bgzf_sets.bgzf(t, block=9000)]
    sets["bgzf_bgzf_no_eof"] = [bgzf_sets.bgzf(fasta(names(b"m", 120), sq(120)), block=5000, eof=False), bgzf_sets.bgzf(t, block=65000)]
    # no final '\n'; a last record that is a header line and nothing else (">x")
    sets["no_final_newline"] = [fastq(names(b"e", 90), sq(90), final_eol=False), fasta(names(b"f", 90), sq(90), final_eol=False), fasta(names(b"g", 5), sq(5))]
    sets["header_only_last"] = [fasta(names(b"h", 60), sq(60)) + b">x", fastq(names(b"i", 60), sq(60))]
    # an empty read in the middle, CRLF, wrapped FASTA
    s = sq(101)
    s[50] = b""
    sets["empty_read"] = [fasta(names(b"j", 101), s), fastq(names(b"k", 101), s)]
    sets["crlf"] = [fasta(names(b"l", 80, b"x"), sq(80), eol=b"\r\n"), fastq(names(b"n", 80), sq(80), eol=b"\r\n")]
    sets["wrapped"] = [fasta(names(b"w", 120), sq(120), wrap=60), fasta(names(b"v", 120), sq(120), wrap=7)]
    # the same name in two files and twice in one file; a name that is a prefix of another
    nm = names(b"r", 150)
    nm[40] = nm[3]
    nm[41] = b"r3"
    nm[42] = b"r"                                            # (a prefix of every other name)
    nm2 = names(b"s", 150)
    nm2[0], nm2[77], nm2[149] = nm[7], nm[40], b"r"
    sets["repeated_names"] = [fastq(nm, sq(150)), fasta(nm2, sq(150))]
    # one file; one long read (the ragged long-row layout)
    sets["one_file"] = [fastq(names(b"o", 210, b"c"), sq(210))]
    s = sq(64)
    s[20] = read(rng, 2100)
    sets["long_read"] = [fasta(names(b"t", 64), s), fasta(names(b"u", 64), sq(64, lo=100, hi=150))]
    # the same length everywhere (the uniform layout) in one file, another in the next: ragged as the host packer makes it
    sets["two_uniform_lengths"] = [fasta(names(b"x", 70), [read(rng, 100) for _ in range(70)]), fasta(names(b"y", 70), [read(rng, 150) for _ in range(70)])]
    return sets


def declined():
    """name -> (files, (file, reason, pos, bgzf reason, bgzf member))"""
    import gzip
    rng = random.Random(77)
    sq = lambda n: [read(rng, l) for l in lens(rng, n)]
    good_a = fasta(names(b"a", 50), sq(50))
    good_q = fastq(names(b"q", 50), sq(50))
    plain_gz = gzip.compress(good_a)
    fq_short = fastq(names(b"b", 20), sq(20))
    lines = fq_short.split(b"\n")[:-1]
    fq_4k1 = b"\n".join(lines[:17]) + b"\n"                 # 4 * 4 + 1 lines: the incomplete record starts at line 16
    pos_4k1 = len(b"\n".join(lines[:16]) + b"\n")
    t = fastq(names(b"z", 120), sq(120))
    members = [bgzf_sets.member(t[i:i + 7000]) for i in range(0, len(t), 7000)]
    bad = bytearray(members[1])
    bad[-8] ^= 0x01                                          # the CRC-32 of member 1
    crc = b"".join([members[0], bytes(bad)] + members[2:]) + bgzf_sets.EOF
    sets = {}
    sets["second_is_plain_gzip"] = ([good_a, plain_gz], (1, 0, 0, bgzf_sets.NOT_BGZF, 0))
    sets["second_fastq_4k_plus_1"] = ([good_q, fq_4k1, good_a], (1, 3, pos_4k1, 0, 0))
    sets["third_bgzf_crc"] = ([good_a, good_q, crc], (2, 0, 0, bgzf_sets.CRC, 1))
    sets["two_offend_first_wins"] = ([good_a, fq_4k1, plain_gz], (1, 3, pos_4k1, 0, 0))
    sets["two_offend_gzip_first"] = ([plain_gz, fq_4k1], (0, 0, 0, bgzf_sets.NOT_BGZF, 0))
    sets["crc_before_scan_offence"] = ([crc, fq_4k1], (0, 0, 0, bgzf_sets.CRC, 1))
    sets["first_byte"] = ([good_a, b"x" + good_a], (1, 2, 0, 0, 0))
    sets["empty_file"] = ([good_q, b""], (1, 1, 0, 0, 0))
    return sets


def verdict_of(lay):
    """a FastxFilesLayout's verdict in the form of declined()"""
    return (lay.decline_file, lay.decline_reason, lay.decline_pos, lay.bgzf[0], lay.bgzf[1])


def text_of(files):
    """every file's text (BGZF inflated by zlib)"""
    import gzip
    return [gzip.decompress(f) if f[:2] == b"\x1f\x8b" else f for f in files]


def joined(files, rec_pos):
    """the arena (every file's text, a line end behind each) and every read's text cut out of it by the scan's own rule"""
    arena = b"".join(t + b"\n" for t in text_of(files))
    reads = []
    for r in range(len(rec_pos) - 1):
        rec = arena[int(rec_pos[r]):int(rec_pos[r + 1])]
        lines = rec.split(b"\n")
        body = lines[1:2] if rec[:1] == b"@" else lines[1:]
        reads.append(bytes(b for l in body for b in l if 33 <= b <= 126))
    return arena, reads


def quality_of(arena, rec_pos, r):
    """the quality string of record r as kseq keeps it (None: a FASTA record)"""
    rec = arena[int(rec_pos[r]):int(rec_pos[r + 1])]
    if rec[:1] != b"@":
        return None
    lines = rec.split(b"\n")
    return bytes(b for b in (lines[3] if len(lines) > 3 else b"") if 33 <= b <= 126)


def write_files(files, directory):
    paths = []
    for k, f in enumerate(files):
        p = directory / ("f%d%s" % (k, ".gz" if f[:2] == b"\x1f\x8b" else ".fx"))
        p.write_bytes(f)
        paths.append(str(p))
    return paths


def edge_sets(tile):
    """files whose boundaries, record starts and quality lines fall on scan tile edges and on 16-byte vector edges.  A tile is `tile`
    bytes counted from the 16-byte aligned address at or below a file's first byte; the arena itself is aligned, so file f's lead
    is its byte base modulo 16."""
    rng = random.Random(4096)
    sets = {}

    def fq(n, name0=b"e0", first=None):
        nm = [name0] + [b"e%d" % i for i in range(1, n)]
        sq = [read(rng, 100 + (i % 5), odd=(i % 13 == 0)) for i in range(n)]
        return fastq(nm, sq)

    def first_file(n_bytes):
        """a FASTA file of exactly n_bytes"""
        t = fasta(names(b"a", 3), [read(rng, 40) for _ in range(3)])
        assert n_bytes > len(t) + 4
        fill = n_bytes - len(t) - 3
        return t + b">p\n" + read(rng, fill - 1) + b"\n"

    def second_with(lead, modulus, what):
        """a FASTQ file in which record 45's header character (what = 0) or the first byte of its quality line (what = 1) lies where
        lead + position is a multiple of modulus: the first record's name is padded until it does"""
        for pad in range(4 * modulus):
            t = fq(60, b"e0" + b"x" * pad)
            pos = [m for m in range(len(t)) if t[m:m + 1] == b"@" and (m == 0 or t[m - 1:m] == b"\n") and t[m:m + 2] == b"@e"][45]
            if what == 1:
                for _ in range(3):
                    pos = t.index(b"\n", pos) + 1
            if (lead + pos) % modulus == 0 and pos > tile:
                return t
        raise AssertionError("no padding puts the position on the edge")

    # every residue of a file's byte base modulo 16 in one set: seventeen files, each a multiple of 16 long, so that with its
    # line end every base is one residue further than the one before
    def fq_multiple_of_16(k):
        for pad in range(200):
            t = fq(3, b"m%d" % k + b"y" * pad)
            if len(t) % 16 == 0:
                return t
        raise AssertionError("no padding")

    sets["every_base_residue"] = [first_file(16 * (10 + k % 3)) if k % 2 == 0 else fq_multiple_of_16(k) for k in range(17)]
    # a file boundary on a tile edge: the first file ends there / the second starts there; a first file far smaller than a tile
    sets["file_ends_on_tile_edge"] = [first_file(tile), fq(20)]
    sets["file_starts_on_tile_edge"] = [first_file(tile - 1), fq(20)]
    sets["two_tiles_then_small"] = [first_file(2 * tile + 5), fasta(names(b"s", 2), [read(rng, 10), read(rng, 0)]), fq(50)]
    sets["tiny_first_file"] = [b">t\nACGT\n", fq(50)]
    for lead in (0, 5, 15):
        n0 = 16 * 9 + lead - 1                                   # (+ 1 for its '\n': the second file's base is lead modulo 16)
        for modulus in (tile, 16):
            for what, tag in ((0, "record"), (1, "quality")):
                sets["%s_on_%d_lead%d" % (tag, modulus, lead)] = [first_file(n0), second_with(lead, modulus, what), bgzf_sets.bgzf(fq(30), block=1500)]
    return sets
