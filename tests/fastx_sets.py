"""Named FASTA / FASTQ files as byte strings, shared by the record scan's tests (test_fastx_scan_host.py,
test_gpu_fastx_scan.py): inputs of the regular class, inputs whose lines and records lie on the device scan's tile edges,
inputs outside the class with the verdict they must get, and a seeded generator of small random files.  Generated data
only; everything is deterministic."""
import random

# decline reasons of include/crass_hip.h
EMPTY, FIRST_BYTE, LINE_COUNT, FQ_HEADER, SEQ_CHAR, FQ_PLUS, QUAL_DEL, QUAL_SHORT, QUAL_LONG, LONE_HEADER = range(1, 11)


def acgt(rng, n):
    return bytes(rng.choices(b"ACGT", k=n))


def fa(name, seq, wrap=0, eol=b"\n", last_eol=True):
    lines = [seq[k:k + wrap] for k in range(0, len(seq), wrap)] if wrap and seq else ([seq] if seq else [])
    body = eol.join(lines) + (eol if lines else b"")
    out = b">" + name + eol + body
    return out if last_eol else out[:len(out) - len(eol)]


def fq(name, seq, qual=None, eol=b"\n", plus=b"+"):
    if qual is None:
        qual = b"I" * len(seq)
    return b"@" + name + eol + seq + eol + plus + eol + qual + eol


def filler_fa(n, tag=b"f"):
    """a FASTA record of exactly n bytes (n >= len(tag) + 3): header, one sequence line"""
    head = b">" + tag + b"\n"
    assert n >= len(head) + 1, n
    return head + b"A" * (n - len(head) - 1) + b"\n"


def filler_fq(n, tag=b"f"):
    """a four-line FASTQ record of exactly n bytes"""
    if (n - len(b"@" + tag + b"\n\n+\n\n")) % 2:
        tag += b"f"
    fixed = len(b"@" + tag + b"\n\n+\n\n")
    assert n >= fixed, n
    k = (n - fixed) // 2
    return fq(tag, b"C" * k)


def regular():
    """name -> bytes, every one inside the regular class"""
    rng = random.Random("fastx_sets:regular")
    d = {}
    recs = [(b"r%d" % i, acgt(rng, rng.randint(1, 200))) for i in range(40)]
    d["one_line"] = b"".join(fa(n, s) for n, s in recs)
    d["wrap60"] = b"".join(fa(n, s, 60) for n, s in recs)
    d["wrap1"] = b"".join(fa(n, s[:40], 1) for n, s in recs[:12])
    d["crlf"] = b"".join(fa(n + b" a comment", s, 60, b"\r\n") for n, s in recs)
    d["empty_lines"] = b"".join(b">" + n + b"\n\n" + s[:30] + b"\n\n\n" + s[30:] + b"\n" for n, s in recs)
    d["no_seq"] = b">first\n" + fa(b"a", recs[0][1]) + b">mid1\n>mid2\n" + fa(b"b", recs[1][1], 60) + b">last\n"
    odd = [b"ACGTNACGT", b"acgtacgtac", b"AC\x00GT", b"AC\xffGT\xfe", b"NNNN", bytes(rng.choices(b"ACGTacgtNU\x00\xff \t\r", k=300)), b"ACGT"]
    d["odd_bytes"] = b"".join(fa(b"o%d" % i, s, 0 if i % 2 else 7) for i, s in enumerate(odd))
    d["header_last_nl"] = d["one_line"] + b">tail with comment\n"
    d["header_last_nonl"] = d["one_line"] + b">tail"
    d["one_record"] = fa(b"only", recs[3][1], 60)
    d["one_header"] = b">x"
    d["no_final_newline"] = b"".join(fa(n, s, 60) for n, s in recs[:5])[:-1]
    d["odd_headers"] = b"".join(fa(h, s) for h, (_, s) in zip([b"a>b", b"a@b +c", b">@+", b"n\tc>omment", b"", b" lead", b"+", b"@"], recs))
    d["dup_names"] = b"".join(fa([b"x", b"y", b"x", b"z", b"y", b"x"][i % 6] + (b" c%d" % i if i % 2 else b""), s) for i, (_, s) in enumerate(recs[:18]))
    d["fq_plain"] = b"".join(fq(n, s, bytes(rng.choices(b"!#5?I~", k=len(s)))) for n, s in recs)
    d["fq_crlf"] = b"".join(fq(n + b" c", s, eol=b"\r\n") for n, s in recs)
    d["fq_no_final_newline"] = d["fq_plain"][:-1]
    d["fq_odd_quality"] = (fq(b"q1", b"ACGT", b"@III") + fq(b"q2", b"ACGT", b"+II@") + fq(b"q3", b"ACGTA", b"II I\tII ") + fq(b"e1", b"", b"") +
                           fq(b"q4", b"AC GT", b"IIII") + fq(b"e2", b"", b" ") + fq(b"q5", b"ACNNT", b">>>>>", plus=b"+q5 again") + fq(b"e3", b"", b"\x80\xff") +
                           fq(b"q6", b"ACGT", b"I\xffI\x01II"))
    d["uniform150"] = b"".join(fa(b"u%d" % i, acgt(rng, 150)) for i in range(300))
    d["fq_uniform150"] = b"".join(fq(b"u%d" % i, acgt(rng, 150)) for i in range(200))
    d["ragged"] = b"".join(fa(b"g%d" % i, acgt(rng, rng.choice([0, 1, 15, 16, 17, 64, 151, rng.randint(1, 700)])), rng.choice([0, 60, 70])) for i in range(150))
    return d


def tile_edge(T):
    """name -> bytes whose lines and records lie on the edges of tiles of T bytes (an aligned buffer: tile k is bytes
    [k T, (k + 1) T)); about 3 T + 100 bytes each"""
    rng = random.Random("fastx_sets:tile_edge")
    total = 3 * T + 100
    d = {}

    def finish_fa(b):
        return b + filler_fa(total - len(b), b"end") if total - len(b) >= 8 else b

    head = fa(b"a", acgt(rng, 77), 60)
    d["hdr_first_byte_of_tile"] = finish_fa(head + filler_fa(T - len(head)) + fa(b"edge", acgt(rng, 90), 60))
    d["hdr_last_byte_of_tile"] = finish_fa(head + filler_fa(T - 1 - len(head)) + fa(b"edge", acgt(rng, 90), 60))
    b = head + b">w\n"
    b += b"G" * (T - 1 - len(b)) + b"\n"                     # '\n' is byte T - 1, the record's next sequence line starts tile 1
    d["nl_last_byte_of_tile"] = finish_fa(b + acgt(rng, 50) + b"\n")
    b = head + b">h"
    b += b"x" * (2 * T - 1 - len(b)) + b"\n"                 # a header line whose '\n' ends tile 1
    d["hdr_nl_last_byte_of_tile"] = finish_fa(b + acgt(rng, 50) + b"\n")
    d["long_header"] = finish_fa(head + (b">" + b"long header " * T)[:2 * T + 4] + b"\n" + acgt(rng, 33) + b"\n")
    d["long_seq_line"] = finish_fa(head + b">s\n" + acgt(rng, 2 * T + 4) + b"\n")
    b = head + filler_fa(T - 40 - len(head)) + b">n\n"
    d["tile_without_newline"] = finish_fa(b + acgt(rng, T + 80) + b"\n" + acgt(rng, 20) + b"\n")
    for name, n in (("exactly_T", T), ("T_minus_1", T - 1), ("T_plus_1", T + 1)):
        d[name] = head + filler_fa(n - len(head))
    d["T_plus_1_name_in_next_tile"] = head + filler_fa(T - 1 - len(head)) + b">z"      # '>' ends tile 0, the name is all of tile 1
    # a FASTQ record whose four lines lie in four tiles, behind one that ends tile 0
    first = filler_fq(T - 10)
    name = b"n" * (T - 1)
    seq = acgt(rng, T)
    d["fq_four_tiles"] = first + fq(name, seq, bytes(rng.choices(b"#5?I@+>", k=T)), plus=b"+" + b"p" * (T - 1)) + fq(b"after", acgt(rng, 40))
    b = fq(b"a", acgt(rng, 30))
    b += filler_fq(T - len(b))
    d["fq_hdr_first_byte_of_tile"] = b + fq(b"edge", acgt(rng, 60)) + fq(b"z", acgt(rng, 41)) * 3
    b = fq(b"ab", acgt(rng, 30))
    b += filler_fq(T - 1 - len(b))
    d["fq_hdr_last_byte_of_tile"] = b + fq(b"edge", acgt(rng, 60)) + fq(b"z", acgt(rng, 2 * T + 5)) + fq(b"y", b"")
    return d


def irregular(T):
    """name -> (bytes, reason, position): inputs outside the regular class, one per decline reason, the offending line in the
    first record, inside the third tile (of T bytes) and in the last record"""
    rng = random.Random("fastx_sets:irregular")
    d = {}

    def place(kind, good, bad_of, reason, fill, wheres=("first", "third_tile", "last")):
        """bad_of() -> (record bytes, offset of the offending line in it); good: a regular record; fill(n): n filler bytes"""
        for where in wheres:
            bad, at = bad_of()
            if where == "first":
                pre = b""
            elif where == "last":
                pre = good * 3
            else:
                pre = good + fill(2 * T + 200 - len(good))
            data = pre + bad + (good * 2 if where != "last" else b"")
            d["%s_%s" % (kind, where)] = (data, reason, len(pre) + at)

    gfa = fa(b"g", acgt(rng, 70), 60)
    gfq = fq(b"g", acgt(rng, 70))
    fill_fq = filler_fq
    place("fa_at_in_seq", gfa, lambda: (b">b\nACGT\nAC@GT\nAC\n", 8), SEQ_CHAR, filler_fa)
    place("fa_plus_line", gfa, lambda: (b">b\nACGT\n+ACGT\n", 8), SEQ_CHAR, filler_fa)
    place("fa_gt_in_seq", gfa, lambda: (b">b\nAC>GT\n", 3), SEQ_CHAR, filler_fa)
    place("fq_qual_short", gfq, lambda: (fq(b"b", b"ACGTAC", b"IIIII"), 12), QUAL_SHORT, fill_fq)
    place("fq_qual_long", gfq, lambda: (fq(b"b", b"ACGTAC", b"IIIIIII"), 12), QUAL_LONG, fill_fq)
    place("fq_qual_del", gfq, lambda: (fq(b"b", b"ACGTAC", b"III\x7fII"), 12), QUAL_DEL, fill_fq)
    place("fq_gt_record", gfq, lambda: (b">b\nACGT\n+\nIIII\n", 0), FQ_HEADER, fill_fq, ("third_tile", "last"))
    d["fa_then_fq_records"] = (b">b\nACGT\n+\nIIII\n" + gfq * 2, SEQ_CHAR, 8)      # byte 0 decides: a FASTA whose third line starts with '+'
    place("fq_no_plus", gfq, lambda: (b"@b\nACGT\n-\nIIII\n", 8), FQ_PLUS, fill_fq)
    place("fq_plus_in_seq", gfq, lambda: (b"@b\nAC+GT\n+\nIIIII\n", 3), SEQ_CHAR, fill_fq)
    place("fq_multi_line", gfq, lambda: (b"@b\nACGT\nACGT\n+\nIIIIIIII\n", 8), FQ_PLUS, fill_fq)
    d["junk_in_front"] = (b"junk\n" + gfa * 2, FIRST_BYTE, 0)
    d["blank_line_in_front"] = (b"\n" + gfa * 2, FIRST_BYTE, 0)
    d["empty_file"] = (b"", EMPTY, 0)
    d["lone_gt_only"] = (b">", LONE_HEADER, 0)
    d["lone_gt_last"] = (gfa * 2 + b">", LONE_HEADER, 2 * len(gfa))
    b = gfa + filler_fa(2 * T + 300 - len(gfa))
    d["lone_gt_third_tile"] = (b + b">", LONE_HEADER, len(b))
    d["fq_4k_plus_1_lines"] = (gfq * 3 + b"@x\n", LINE_COUNT, 3 * len(gfq))
    d["fq_trailing_blank_line"] = (gfq * 3 + b"\n", LINE_COUNT, 3 * len(gfq))
    b = gfq + fill_fq(2 * T + 200 - len(gfq))
    d["fq_truncated_third_tile"] = (b + b"@t\nACGT\n+\n", LINE_COUNT, len(b))
    d["fq_truncated_no_newline"] = (gfq + b"@t\nACGT\n+", LINE_COUNT, len(gfq))
    d["fq_one_line"] = (b"@", LINE_COUNT, 0)
    return d


def in_regular_class(data):
    """the regular class of include/crass_hip.h, restated line by line"""
    if not data or data[:1] not in (b">", b"@"):
        return False
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    bad = set(b">@+")
    graph = lambda s: sum(1 for c in s if 33 <= c <= 126)
    if data[:1] == b">":
        if data.endswith(b">") and (len(data) == 1 or data[-2:-1] == b"\n"):
            return False
        return all(ln[:1] == b">" or not (set(ln) & bad) for ln in lines)
    if len(lines) % 4:
        return False
    for k in range(0, len(lines), 4):
        h, s, p, q = lines[k:k + 4]
        if h[:1] != b"@" or (set(s) & bad) or p[:1] != b"+" or 127 in q or graph(q) != graph(s):
            return False
    return True


def reads_by_rule(data, rec_pos):
    """the reads of an accepted input from its record positions: the bytes 33..126 of every record's sequence lines"""
    out = []
    fastq = data[:1] == b"@"
    for r in range(len(rec_pos) - 1):
        lines = data[int(rec_pos[r]):int(rec_pos[r + 1])].split(b"\n")
        body = lines[1:2] if fastq else lines[1:]
        out.append(bytes(c for ln in body for c in ln if 33 <= c <= 126))
    return out


def random_input(rng):
    """one small random file: FASTA or FASTQ, wrapped or not, LF or CRLF, empty reads, a header as the last line, quality lines
    that start with '@' or hold blanks; one draw in seven gets a single-byte mutation"""
    fastq = rng.random() < 0.45
    eol = b"\r\n" if rng.random() < 0.2 else b"\n"
    parts = []
    for i in range(rng.randint(1, 8)):
        L = rng.choice([0, 1, 2, 5, 16, 17, rng.randint(0, 80)])
        seq = bytes(rng.choices(b"ACGTNacgt" if rng.random() < 0.3 else b"ACGT", k=L))
        name = bytes(rng.choices(b"abcxyz019_>@+", k=rng.randint(0, 6)))
        if rng.random() < 0.3:
            name += rng.choice([b" ", b"\t"]) + bytes(rng.choices(b"comment >@+ ", k=rng.randint(0, 8)))
        if fastq:
            q = bytearray(rng.choices(b"!#5?I~@+>", k=L))
            if L and rng.random() < 0.15:
                q.insert(rng.randrange(L + 1), rng.choice(b" \t"))
            plus = b"+" + (name if rng.random() < 0.2 else b"")
            parts.append(b"@" + name + eol + seq + eol + plus + eol + bytes(q) + eol)
        else:
            wrap = rng.choice([0, 0, 1, 7, 60])
            lines = [seq[k:k + wrap] for k in range(0, len(seq), wrap)] if wrap and seq else ([seq] if seq or rng.random() < 0.5 else [])
            if lines and rng.random() < 0.1:
                lines.insert(rng.randrange(len(lines) + 1), b"")
            parts.append(b">" + name + eol + b"".join(ln + eol for ln in lines))
    data = b"".join(parts)
    if not fastq and rng.random() < 0.15:
        data += b">" + bytes(rng.choices(b"tail", k=rng.randint(1, 4)))      # a header as the last line, without its '\n'
    elif rng.random() < 0.25:
        data = data[:len(data) - len(eol)]                                    # no final newline
    if rng.random() < 1 / 7:
        b = bytearray(data)
        how = rng.random()
        at = rng.randrange(len(b))
        if how < 0.6:
            b[at] = rng.choice(b">@+\n\r A\x7f\x00\xff-")
        elif how < 0.8:
            del b[at]
        else:
            b.insert(at, rng.choice(b">@+\n I"))
        data = bytes(b)
    return data
