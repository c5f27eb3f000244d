"""The cut rule of csrc/fastx_scan.h (record-aligned shards of a job's files) stated by brute force, and the designed inputs of
tests/test_fastx_shards_host.py and tests/test_gpu_group_fastx_files.py.

brute_shards lists EVERY line start of every file's text and picks: the job's text space is the texts back to back; a record
start is a file's position 0, every line start whose byte is '>' in a file whose byte 0 is '>', every line start of line index
0 modulo 4 in a file whose byte 0 is '@'; the actual cut is the smallest record start at or after the nominal one, or T."""
import bisect
import random

from tests import bgzf_sets, files_sets

TILE = 4096


def record_starts(text):
    ls = [0] + [i + 1 for i, b in enumerate(text) if b == 10 and i + 1 < len(text)]
    if text[:1] == b">":
        return [p for p in ls if text[p] == 0x3E]
    if text[:1] == b"@":
        return [p for k, p in enumerate(ls) if k % 4 == 0]
    return [0]


def text_bases(files):
    tb = [0]
    for t in files_sets.text_of(files):
        tb.append(tb[-1] + len(t))
    return tb


def default_nominal(files, n_ranks):
    T = text_bases(files)[-1]
    return [T * g // n_ranks for g in range(1, n_ranks)]


def brute_shards(files, n_ranks, nominal=None):
    """-> (cuts [(file, pos)] * (n_ranks + 1), rank_read_base [n_ranks + 1])"""
    texts = files_sets.text_of(files)
    tb = text_bases(files)
    T = tb[-1]
    starts = [tb[f] + p for f, t in enumerate(texts) for p in record_starts(t)]
    nominal = default_nominal(files, n_ranks) if nominal is None else list(nominal)
    cuts, base = [], []
    for x in [0] + nominal + [T]:
        k = bisect.bisect_left(starts, x)
        base.append(k)
        if k == len(starts):
            cuts.append((len(files), 0))
        else:
            f = bisect.bisect_right(tb, starts[k]) - 1
            cuts.append((f, starts[k] - tb[f]))
    return cuts, base


# ---- designed inputs ----
def small_fastq():
    """about 200 bytes; record 2's quality line starts with '@', record 1's with '+', a header holds '>' and '@'"""
    return (b"@q0 c\nACGTACGTAC\n+\nIIIIIIIIII\n"
            b"@q1>x@y\nACGTNACG\n+\n+IIIIIII\n"
            b"@q2\nTTGACCA\n+\n@IIIIII\n"
            b"@q3\nA\n+\nI\n"
            b"@q0 again\nACGTACGTACGTACGTACGTACGTACGTAC\n+\n@@@@@@@@@@@@@@@@@@@@@@@@@@@@@@\n"
            b"@q5\nGGGGCCCCAAAATTTT\n+\n>>>>>>>>>>>>>>>>\n")


def small_fasta():
    """about 200 bytes, multi-line records, '>' and '@' inside header text, an empty record"""
    return (b">a0 first>second@third\nACGTACGTACGTACGTACGT\nACGTACGT\n"
            b">a1\nTTTTGGGGCCCCAAAATTTTGGGGCCCCAAAA\nAC\nG\n"
            b">a2\n"
            b">q2 same name as a fastq read\nNNNNACGT\nACGTNACGTACGTACGTACGTACGTACG\n"
            b">a4\nGATTACAGATTACAGATTACA\nGATTACA\n")


def tile_edge_fastq(edge, rng):
    """a FASTQ whose record 1 starts at text position `edge`: record 0 is one long read; a few records behind it"""
    n = (edge - len(b"@long\n\n+\n\n")) // 2
    pad = edge - (2 * n + len(b"@long\n\n+\n\n"))
    s = files_sets.read(rng, n)
    t = b"@long" + b"x" * pad + b"\n" + s + b"\n+\n" + b"I" * n + b"\n"
    assert len(t) == edge
    nm = files_sets.names(b"t", 40)
    return t + files_sets.fastq(nm, [files_sets.read(rng, 90 + i % 7, odd=(i % 5 == 0)) for i in range(40)])


def cases():
    """name -> (files, positions): every position is to be a nominal cut of some rank (text space); None stands for the even cuts"""
    rng = random.Random(2121)
    out = {}
    fq, fa = small_fastq(), small_fasta()
    q = fq.index(b"\n@IIIIII") + 1                       # the quality line that starts with '@'
    out["quality_line_starts_with_at"] = ([fq], [q - 1, q, q + 1])
    out["header_chars_inside_headers"] = ([fq, fa], [fq.index(b">x@y"), fq.index(b"@y"), len(fq) + fa.index(b">second"), len(fq) + fa.index(b"@third")])
    crlf = files_sets.fastq(files_sets.names(b"c", 6), [files_sets.read(rng, 20 + i) for i in range(6)], eol=b"\r\n")
    cr = crlf.index(b"\r\n", 60)
    out["newline_cr_and_file_boundary"] = ([crlf, fa], [cr, cr + 1, cr + 2, len(crlf) - 1, len(crlf), len(crlf) + 1, fq.index(b"\n")])
    nf = files_sets.fasta(files_sets.names(b"n", 5), [files_sets.read(rng, 30) for _ in range(5)], final_eol=False)
    out["last_line_without_newline"] = ([fq[:-1], nf], [len(fq) - 3, len(fq) - 2, len(fq) - 1, len(fq) - 1 + len(nf) - 2, len(fq) - 1 + len(nf) - 1, len(fq) - 1 + len(nf)])
    long_rec = b">short\nACGT\n>long one\n" + b"\n".join(files_sets.read(rng, 60) for _ in range(20)) + b"\n>tail\nAC\n"
    out["record_longer_than_a_range"] = ([long_rec], [None, 100, 400, 700, 1000])
    out["more_ranks_than_records"] = ([b">only\nACGT\n", b"@two\nAC\n+\nII\n"], [None, 1, 5, 11, 12])
    t3 = files_sets.fastq(files_sets.names(b"z", 60, b"lane"), [files_sets.read(rng, l, odd=(i % 7 == 0)) for i, l in enumerate(files_sets.lens(rng, 60))])
    three = [fa, fq, bgzf_sets.bgzf(t3, block=1500)]
    out["fasta_fastq_bgzf"] = (three, [None, len(fa), len(fa) + len(fq), len(fa) + len(fq) + 1, len(fa) + len(fq) + 1499, len(fa) + len(fq) + 1500, len(fa) + len(fq) + 3001])
    # BGZF: members of 1000 text bytes — records straddle them; cuts inside the second member, on member boundaries, in the last
    tb = files_sets.fastq(files_sets.names(b"b", 40), [files_sets.read(rng, 100 + i % 9) for i in range(40)])
    out["bgzf_straddling_members"] = ([bgzf_sets.bgzf(tb, block=1000)], [None, 999, 1000, 1001, 1500, 2000, 2001, len(tb) - 10])
    # exception reads (an N) on both sides of a cut
    ex = files_sets.fastq(files_sets.names(b"x", 12), [files_sets.read(rng, 50)[:25] + b"N" + files_sets.read(rng, 24) for _ in range(12)])
    mid = [i for i in range(len(ex)) if ex[i:i + 1] == b"@" and (i == 0 or ex[i - 1:i] == b"\n") and ex[i:i + 2] == b"@x"][6]
    out["exception_reads_around_the_cut"] = ([ex], [mid - 1, mid, mid + 1])
    # the probe's tile and vector edges: the record start the cut must find lies on / around a tile edge and a 16-byte boundary of
    # the staged range, whose start takes every alignment 0 .. 15 (the staged bytes lie at their text position modulo 16)
    for edge in (TILE - 1, TILE, TILE + 1, TILE + 15, TILE + 16, TILE + 17, 2 * TILE):
        out["tile_edge_%d" % edge] = ([tile_edge_fastq(edge, rng)], list(range(1, 17)) + [edge - 1, edge, edge + 1])
    return out


def nominal_lists(files, positions, n_ranks):
    """the positions as nominal cut lists for n_ranks: sorted chunks of n_ranks - 1 (the last chunk repeats its last position)"""
    lists = []
    if None in positions:
        lists.append(None)
    if all(p is None for p in positions):                # (a file that does not inflate has no text to measure)
        return lists
    T = text_bases(files)[-1]
    pos = sorted(min(p, T) for p in positions if p is not None)
    k = n_ranks - 1
    for i in range(0, len(pos), k):
        chunk = pos[i:i + k]
        lists.append(chunk + [chunk[-1]] * (k - len(chunk)))
    return lists


def declined():
    """name -> (files, positions): small inputs the scan declines, with cuts at, before and behind the offence"""
    fq, fa = small_fastq(), small_fasta()
    out = {}
    h = fq.index(b"@q3")
    out["fastq_header_lacks_at_on_the_cut"] = ([fa, fq[:h] + b"X" + fq[h + 1:]], [len(fa) + h - 1, len(fa) + h, len(fa) + h + 1, len(fa) + 5, len(fa) + len(fq) - 5])
    last = fq.rindex(b"@q5")
    cutoff = fq.index(b"\n", fq.index(b"\n", last) + 1) + 1          # two lines of the last record
    out["incomplete_last_record"] = ([fq[:cutoff]], [last - 1, last, last + 1, cutoff - 2, 10])
    out["lone_header_at_the_end"] = ([fa + b">"], [len(fa) - 1, len(fa), len(fa) + 1, 30])
    out["quality_short_in_second_part"] = ([fq.replace(b"@IIIIII\n", b"@IIIII\n")], [20, fq.index(b"@q2"), fq.index(b"@q3")])
    out["junk_first_byte_second_file"] = ([fq, b"x" + fa], [10, len(fq), len(fq) + 1])
    assert fa.endswith(b"\nGATTACA\n")
    out["plus_in_the_last_sequence_line"] = ([fa[:-8] + b"GAT+ACA\n"], [50, 150])
    return out
