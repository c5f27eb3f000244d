"""Named wrapped FASTQ files as byte strings, shared by the wrapped scan's tests (test_wrapped_scan_host.py,
test_gpu_wrapped_scan.py, test_gpu_wrapped_quality.py): inputs of the class with every shape the rule names, inputs outside it
with the verdict they must get, the rule restated in Python, and a seeded generator that draws from the class's grammar.
Generated data only; everything is deterministic."""
import random

from tests.fastx_sets import acgt, filler_fq, fq

# decline reasons of include/crass_hip.h
NO_PLUS, NOT_HEADER, SEQ_CHAR, QUAL_DEL, QUAL_SHORT, QUAL_LONG, EMPTY_SEQ = 3, 4, 5, 7, 8, 9, 12


def wrap(s, w):
    return [s[k:k + w] for k in range(0, len(s), w)] if w and s else ([s] if s else [])


def wfq(name, seq, qual=None, w=60, qw=None, eol=b"\n", plus=b"+", after=()):
    """one record: the sequence in lines of w bytes, the quality in lines of qw (default w), the void lines `after` behind it"""
    if qual is None:
        qual = b"I" * len(seq)
    lines = [b"@" + name] + wrap(seq, w) + [plus] + wrap(qual, w if qw is None else qw) + list(after)
    return b"".join(ln + eol for ln in lines)


def judge(data):
    """the wrapped rule of include/crass_hip.h restated line by line: (reason, position, rec_pos, reads); reason 0: accepted"""
    if not data:
        return 1, 0, [], []
    if data[:1] != b"@":
        return 2, 0, [], []
    lines, p = [], 0
    while p < len(data):
        e = data.find(b"\n", p)
        lines.append((p, data[p:len(data) if e < 0 else e], e >= 0))
        p = len(data) if e < 0 else e + 1
    graph = lambda s: sum(1 for c in s if 33 <= c <= 126)
    is_void = lambda s: not any(33 <= c <= 127 for c in s)
    rec_pos, reads, i, n = [], [], 0, len(lines)
    while i < n:
        hdr = lines[i][0]
        j = i + 1
        while j < n and lines[j][1][:1] != b"+":
            j += 1
        if j == n:
            return NO_PLUS, hdr, [], []
        for k in range(i + 1, j):
            if set(lines[k][1]) & set(b">@+"):
                return SEQ_CHAR, lines[k][0], [], []
        read = bytes(c for k in range(i + 1, j) for c in lines[k][1] if 33 <= c <= 126)
        if not read and j + 1 < n and lines[j + 1][1][:1] == b"@":
            return EMPTY_SEQ, lines[j + 1][0], [], []
        q, count = j + 1, 0
        if lines[j][2]:
            while count < len(read) and q < n:
                count += graph(lines[q][1])
                q += 1
        for k in range(j + 1, q):
            if 127 in lines[k][1]:
                return QUAL_DEL, lines[k][0], [], []
        if count > len(read):
            return QUAL_LONG, lines[q - 1][0], [], []
        if not lines[j][2] or count < len(read):
            return QUAL_SHORT, hdr, [], []
        while q < n and is_void(lines[q][1]):
            q += 1
        if q < n and lines[q][1][:1] != b"@":
            return NOT_HEADER, lines[q][0], [], []
        rec_pos.append(hdr)
        reads.append(read)
        i = q
    return 0, 0, rec_pos + [len(data)], reads


def records(data):
    """(name line, read, quality) of every record of an accepted input, from the rule"""
    reason, _, rec_pos, reads = judge(data)
    assert reason == 0, reason
    out = []
    for r, read in enumerate(reads):
        lines = data[rec_pos[r]:rec_pos[r + 1]].split(b"\n")
        j = next(k for k in range(1, len(lines)) if lines[k][:1] == b"+")
        qual = bytes(c for ln in lines[j + 1:] for c in ln if 33 <= c <= 126)[:len(read)]
        out.append((lines[0][1:].rstrip(b"\r"), read, qual))
    return out


def unwrapped(data):
    """the same records as a four-line FASTQ"""
    return b"".join(fq(name, read, qual) for name, read, qual in records(data))


def n_records(n, seed="n"):
    """n wrapped records of 0 .. 11 bases in lines of 4, a blank line now and then"""
    rng = random.Random("wrapped_sets:%s:%d" % (seed, n))
    parts = []
    for i in range(n):
        L = rng.randint(1, 11) if i % 97 else 0
        parts.append(wfq(b"r%d" % i, acgt(rng, L), bytes(rng.choices(b"!5I~@+", k=L)), w=4, after=(b"",) if L == 0 or i % 5 == 0 else ()))
    return b"".join(parts)


COUNTS = (1, 2, 3, 63, 64, 65, 1023, 1025, 70001)


def at_offset(rec, line_in_rec, target, tail):
    """rec behind four-line filler records so that its line number line_in_rec starts at byte `target`"""
    off = sum(len(ln) + 1 for ln in rec.split(b"\n")[:line_in_rec])
    return filler_fq(target - off) + rec + tail


def designed(T):
    """name -> bytes, every one inside the wrapped class (and none but the last two inside the four-line class)"""
    rng = random.Random("wrapped_sets:designed")
    d = {}
    recs = [(b"r%d" % i, acgt(rng, rng.randint(1, 200))) for i in range(24)]
    qual = lambda s: bytes(rng.choices(b"!#5?I~", k=len(s)))
    for w in (1, 7, 60):
        d["wrap%d" % w] = b"".join(wfq(n, s[:40 if w == 1 else 200], w=w) for n, s in recs[:10 if w == 1 else 24])
    for L in (T - 1, T, T + 1):
        d["line_of_%d" % L] = wfq(b"a", acgt(rng, 30), w=7) + wfq(b"long", acgt(rng, 2 * L + 5), w=L) + wfq(b"z", acgt(rng, 9), w=4)
    d["one_base"] = wfq(b"one", b"A", b"#") + b"\n"
    d["one_base_wrapped_neighbours"] = wfq(b"a", acgt(rng, 9), w=4) + wfq(b"one", b"G") + wfq(b"z", acgt(rng, 9), w=4)
    d["quality_starts_with_at_and_plus"] = b"".join(wfq(n, s[:24], (b"@II+II" * 4)[:len(s[:24])], w=8, qw=3) for n, s in recs[:8])
    d["plus_repeats_name"] = b"".join(wfq(n, s, w=50, plus=b"+" + n) for n, s in recs[:8])
    d["crlf"] = b"".join(wfq(n + b" comment", s, qual(s), w=60, eol=b"\r\n", after=(b"",) if i % 3 == 0 else ()) for i, (n, s) in enumerate(recs[:9]))
    d["void_lines"] = b"".join(wfq(n, s, w=33, after=[(), (b"",), (b"\r",), (b"  ", b"\t"), (b"", b"\x80\xff", b"")][i % 5]) for i, (n, s) in enumerate(recs[:10])) + b"\n \n"
    d["void_lines_inside"] = b"@a\n\nAC\n\r\nGT\n\n+\n\nII\n \nII\n@b\nA\n+\nI\n"
    d["blanks_in_lines"] = b"@a c\nAC GT\n A\tC\n+\nII II\nI I\n@b\nA\n+\nI\n"
    d["empty_then_void"] = wfq(b"a", b"ACGT", w=2) + b"@e\n+\n\n" + wfq(b"b", b"AC", w=1) + b"@e2\n\n+\n \n" + wfq(b"c", b"A")
    d["empty_at_end"] = wfq(b"a", b"ACGT", w=2) + b"@e\n+\n"
    d["empty_only"] = b"@e\n+\n"
    d["trailing_blank_line"] = fq(b"a", b"ACGT") + fq(b"b", b"AC") + b"\n"
    d["no_final_newline"] = wfq(b"a", acgt(rng, 50), w=20)[:-1]
    d["read_9000_wrap60"] = wfq(b"a", acgt(rng, 30), w=7) + wfq(b"long", acgt(rng, 9000), bytes(rng.choices(b"!5I~@+>", k=9000)), w=60) + wfq(b"z", acgt(rng, 9), w=4)
    # header, '+' and quality lines on a tile's first and last byte
    rec = wfq(b"edge", acgt(rng, 90), (b"@+I" * 30), w=30)      # lines: 0 header, 1..3 sequence, 4 '+', 5..7 quality
    tail = wfq(b"z", acgt(rng, 9), w=4)
    for what, line in (("hdr", 0), ("plus", 4), ("qual", 5), ("qual2", 6)):
        d["%s_first_byte_of_tile" % what] = at_offset(rec, line, T, tail)
        d["%s_last_byte_of_tile" % what] = at_offset(rec, line, 2 * T - 1, tail)
    for n in COUNTS:
        d["records_%d" % n] = n_records(n)
    # every quality line starts with '@'; read as headers, the lines behind them would offend (no '+' line, '>' in a sequence
    # line, a quality that passes its sequence, junk behind it)
    parts = []
    for i in range(40):
        s = acgt(rng, 12)
        parts.append(b"@r%d\n" % i + s[:6] + b"\n" + s[6:] + b"\n+\n@IIII>\n@+III~\n" + (b"\n" if i % 2 else b""))
    d["quality_lines_look_like_headers"] = b"".join(parts)
    # inside the four-line class as well
    d["four_line"] = b"".join(fq(n, s, qual(s)) for n, s in recs)
    d["four_line_empty_reads"] = fq(b"a", b"ACGT") + fq(b"e", b"", b"") + fq(b"b", b"AC") + fq(b"e2", b"", b" ")
    return d


FOUR_LINE = ("four_line", "four_line_empty_reads")


def declines(T):
    """name -> (bytes, reason, position): outside the class, each reason in the first record, in the third tile and in the last"""
    rng = random.Random("wrapped_sets:declines")
    d = {}
    good = wfq(b"g", acgt(rng, 70), w=30)
    cases = {
        "no_plus": (b"@b\nACGT\nACGT\n", NO_PLUS, 0),
        "gt_in_seq": (b"@b\nACGT\nAC>T\nAC\n+\nIIIIIIIIII\n", SEQ_CHAR, 8),
        "at_line_in_seq": (b"@b\nACGT\n@CGT\n+\nIIIIIIII\n", SEQ_CHAR, 8),
        "empty_then_at": (b"@b\n+\n@c\nA\n+\nI\n", EMPTY_SEQ, 5),
        "qual_del": (b"@b\nACGT\nAC\n+\nIII\nI\x7fII\n", QUAL_DEL, 17),
        "qual_passes": (b"@b\nACGT\nAC\n+\nIII\nIIII\n", QUAL_LONG, 17),
        "not_header": (b"@b\nACGT\n+\nIIII\n\nACGT\n+\nIIII\n", NOT_HEADER, 16),
        "gt_record": (b"@b\nACGT\n+\nIIII\n>c\nACGT\n", NOT_HEADER, 15),
    }
    for kind, (bad, reason, at) in cases.items():
        last_only = kind in ("no_plus",)                 # (what follows would supply the missing line)
        for where in ("first", "third_tile", "last"):
            if last_only and where != "last":
                continue
            pre = b"" if where == "first" else good * 3 if where == "last" else good + filler_fq(2 * T + 200 - len(good))
            d["%s_%s" % (kind, where)] = (pre + bad + (good * 2 if where != "last" and not last_only else b""), reason, len(pre) + at)
    d["qual_short_last"] = (good * 2 + b"@b\nACGT\nAC\n+\nIII\nII\n", QUAL_SHORT, 2 * len(good))
    d["qual_short_no_quality"] = (good + b"@b\nACGT\n+\n", QUAL_SHORT, len(good))
    d["plus_ends_input"] = (good + b"@b\nACGT\n+", QUAL_SHORT, len(good))
    d["empty_plus_ends_input"] = (good + b"@e\n+", QUAL_SHORT, len(good))
    bad = b"@b\nACGTACGTACGT\n+\nII\n"                  # the count goes on through the next record's header and passes in its sequence
    d["qual_short_swallows_records"] = (bad + good * 2, QUAL_LONG, len(bad) + good.index(b"\n") + 1)
    d["header_only"] = (b"@", NO_PLUS, 0)
    d["junk_in_front"] = (b"\n" + good, 2, 0)
    d["empty_file"] = (b"", 1, 0)
    return d


VOID = (b"", b"", b" ", b"\t", b"  \t", b"\x80\xff", b"\x00")


def generate(rng):
    """one small file drawn from the class's grammar; asserts its own membership by judge()"""
    eol = b"\r\n" if rng.random() < 0.2 else b"\n"
    void = lambda: rng.choice(VOID)
    lines = []
    n = rng.randint(1, 7)
    for i in range(n):
        name = bytes(rng.choices(b"abcxyz019_>@+", k=rng.randint(0, 6)))
        if rng.random() < 0.3:
            name += rng.choice([b" ", b"\t"]) + bytes(rng.choices(b"comment >@+ ", k=rng.randint(0, 8)))
        lines.append(b"@" + name)
        L = rng.choice([0, 1, 2, 5, 16, 17, rng.randint(0, 80)])
        seq = bytes(rng.choices(b"ACGTNacgt" if rng.random() < 0.3 else b"ACGT", k=L))
        for chunk in wrap(seq, rng.choice([0, 1, 3, 7, 60])):
            if rng.random() < 0.1:
                lines.append(void())
            if rng.random() < 0.1 and len(chunk) > 1:
                chunk = chunk[:1] + rng.choice([b" ", b"\t", b"\x00"]) + chunk[1:]
            lines.append(chunk)
        lines.append(b"+" + (name if rng.random() < 0.2 else bytes(rng.choices(b"+@> x", k=rng.randint(0, 3)))))
        qual = bytes(rng.choices(b"!#5?I~@+>", k=L))
        for chunk in wrap(qual, rng.choice([0, 1, 3, 7, 60])):
            if rng.random() < 0.1:
                lines.append(void())
            if rng.random() < 0.1 and len(chunk) > 1:
                chunk = chunk[:1] + rng.choice([b" ", b"\t"]) + chunk[1:]
            lines.append(chunk)
        n_void = rng.choice([0, 0, 0, 1, 2])
        if L == 0 and i + 1 < n:
            n_void = max(n_void, 1)                      # (an '@' right behind the '+' line of an empty sequence is reason 12)
        lines += [void() for _ in range(n_void)]
    data = b"".join(ln + eol for ln in lines)
    if rng.random() < 0.25 and lines[-1][:1] != b"+":
        data = data[:-1]                                 # no final '\n' (behind a '+' line the input would end inside it)
    assert judge(data)[0] == 0, data
    return data


def mutate(rng, data):
    b = bytearray(data)
    how, at = rng.random(), rng.randrange(len(b))
    if how < 0.6:
        b[at] = rng.choice(b">@+\n\r A\x7f\x00\xff-I")
    elif how < 0.8:
        del b[at]
    else:
        b.insert(at, rng.choice(b">@+\n I\x7f"))
    return bytes(b)
