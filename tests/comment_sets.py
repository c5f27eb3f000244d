"""Designed FASTA / FASTQ jobs for the comment kseq hands on from record to record (csrc/fastx_scan.h: a record without a comment
of its own is handed the last one seen earlier in the SAME file, a record in front of its file's first comment none).  Every job
is a list of files of the regular class (crass_fastx_scan_host accepts each one); jobs() maps a name to that list.  model() is
the rule restated by one forward walk per file over header LINES, as kseq's buffer carries it — the tests use it only to say
what a set is (how many records are handed a comment that is not on their own line); the pinned reference of the host function
is crass_read_fastx, that of the device the host function."""
import random

SPACE = b" \t\n\v\f\r"


def fasta(headers, eol=b"\n", seq=b"ACGT", open_end=False):
    """two-line records from header lines (without '>'); open_end: the last header line is the file's end, without its line end"""
    out = []
    for i, h in enumerate(headers):
        if open_end and i + 1 == len(headers):
            out.append(b">" + h)
        else:
            out.append(b">" + h + eol + seq + eol)
    return b"".join(out)


def fastq(headers, eol=b"\n", seq=b"ACGTAC"):
    return b"".join(b"@" + h + eol + seq + eol + b"+" + eol + b"I" * len(seq) + eol for h in headers)


def headers(n, every, first=0, tag=b"r", comment=lambda r: b"c%d x" % (r * 7)):
    """n names tag<r>; a comment on record first, first + every, ... (every == 0: on none)"""
    return [tag + b"%d" % r + (b" " + comment(r) if every and r >= first and (r - first) % every == 0 else b"") for r in range(n)]


def jobs():
    J = {}
    J["every_third"] = [fasta(headers(30, 3))]
    J["every_third_fq"] = [fastq(headers(31, 3, 1))]
    J["none"] = [fasta(headers(30, 0))]
    J["all"] = [fasta(headers(30, 1))]
    J["late_first"] = [fasta(headers(30, 4, 9))]
    J["empty_own"] = [fasta([b"a first", b"b ", b"c", b"d\t", b"e", b"f second", b"g\r", b"h", b"i \t ", b"j"])]
    J["crlf"] = [fasta(headers(20, 2, 1), eol=b"\r\n")]
    J["crlf_fq"] = [fastq(headers(20, 3, 2), eol=b"\r\n")]
    J["long_comment"] = [fasta([b"a", b"b " + b"x" * 300, b"c", b"d"])]
    J["long_names"] = [fasta([b"z zero", b"a" * 259, b"b" * 259 + b" c259", b"c" * 260, b"d" * 260 + b"\tc260", b"e" * 300, b"f" * 300 + b" c300", b"y"])]
    J["open_end_comment"] = [fasta([b"a", b"b c", b"c", b"last tail comment"], open_end=True)]
    J["open_end_none"] = [fasta([b"a", b"b c", b"c", b"last"], open_end=True)]
    J["open_end_blank"] = [fasta([b"a", b"b c", b"c", b"last "], open_end=True)]
    J["one_commented"] = [fasta([b"only one"])]
    for n in (1, 63, 64, 65, 4095, 4096, 4097):
        J["count_%d" % n] = [fasta(headers(n, 5, 2), seq=b"A")]
    sparse = [b"r"] * 12300
    sparse[4095] = b"r only"
    J["sparse"] = [fasta(sparse, seq=b"A")]
    J["two_files"] = [fasta(headers(10, 1, tag=b"a")), fasta(headers(10, 0, tag=b"b"))]
    J["three_files"] = [fasta(headers(100, 3, 2, tag=b"a")), fastq(headers(50, 0, tag=b"b")), fasta(headers(70, 4, 5, tag=b"c"))]
    J["open_end_between"] = [fasta([b"a c", b"b"], open_end=True), fasta([b"d", b"e f", b"g"])]
    return J


SPARSE_QUERIES = [4095, 4096, 8191, 8192, 12299, 4094, 0]


def arena(files):
    """the bytes of a job as crass_hip_load_fastx_files lays them out: every file's text with a '\\n' behind it"""
    return b"".join(f + b"\n" for f in files)


def model(files):
    """per record of the job, in order: (has, comment, own) — own: the comment is on the record's own header line"""
    out = []
    for text in files:
        lines = text.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        fq = text[:1] == b"@"
        have, carried = False, b""
        for i, line in enumerate(lines):
            if (i % 4 != 0) if fq else (line[:1] != b">"):
                continue
            body = line[1:]
            e = 0
            while e < len(body) and body[e] not in SPACE:
                e += 1
            if e < len(body):
                have, carried = True, body[e + 1:]
            out.append((1 if have else 0, carried if have else b"", e < len(body)))
    return out


def picks(name, n):
    """record numbers in any order, with repeats, every record at least once"""
    rng = random.Random("comments:" + name)
    idx = list(range(n)) + [rng.randrange(n) for _ in range(min(n, 200) + 5)]
    rng.shuffle(idx)
    return idx


def concat(items):
    import numpy as np
    off = np.zeros(len(items) + 1, np.uint64)
    for k, b in enumerate(items):
        off[k + 1] = off[k] + np.uint64(len(b))
    return np.frombuffer(b"".join(items), np.uint8), off
