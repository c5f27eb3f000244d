"""Designed FASTA / FASTQ texts and query lists for the lookup of names (crass_fastx_find_names on the host,
crass_hip_fastx_names_find on the device; test_find_names_host.py, test_gpu_find_names.py), with the rule restated as a Python
dictionary.  Generated data only; everything is deterministic.  A text comes with the positions of its records' header
characters, so that texts outside the record scan's regular class can be used too."""
import random

import numpy as np

from tests.fastx_sets import acgt, fa, fq

SPACE = b" \t\n\x0b\x0c\r"
NOT_FOUND = 2 ** 64 - 1
LENGTHS = (0, 1, 3, 4, 5, 8, 259, 260, 261, 1000)      # around a dword, around where a name goes from a lane to a wave, far beyond
ALPHABET = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_/.:#|>@+-"


def rand_name(rng, n):
    return bytes(rng.choices(ALPHABET, k=n))


def build(recs):
    """records -> (the text, uint64 positions of the header characters with the text's size behind them)"""
    pos, data = [], b""
    for r in recs:
        pos.append(len(data))
        data += r
    return data, np.asarray(pos + [len(data)], np.uint64)


def name_at(data, p):
    a = b = p + 1
    while b < len(data) and data[b] not in SPACE:
        b += 1
    return data[a:b]


def first_by_name(data, rec_pos):
    """{name: the smallest record index with it}: the rule"""
    d = {}
    for r in range(len(rec_pos) - 1):
        d.setdefault(name_at(data, int(rec_pos[r])), r)
    return d


def expected(data, rec_pos, queries):
    d = first_by_name(data, rec_pos)
    return np.asarray([d.get(bytes(q), NOT_FOUND) for q in queries], np.uint64)


def other(b):
    return b"!" if b != b"!" else b"?"


def variants(nm):
    """a name with one byte changed (the first, the last), one byte longer, one byte shorter"""
    out = [nm + b"x", nm + b"\x00"]
    if nm:
        out += [nm[:-1] + other(nm[-1:]), other(nm[:1]) + nm[1:], nm[:-1]]
    if len(nm) > 8:
        out += [nm[:5] + other(nm[5:6]) + nm[6:], nm[1:]]
    return out


def queries(data, rec_pos):
    """every present name, its variants, absent and empty queries, queries with an isspace() byte, duplicates"""
    names = list(first_by_name(data, rec_pos))
    q = list(names)
    for nm in names:
        q += variants(nm)
    q += [b"", b"no-such-name", b"has space", b"tab\tinside", b" ", b"\n", b"trailing ", b" leading", b"x" * 300 + b" " + b"y" * 10, b"z" * 259 + b"\t"]
    q += [nm + b" " for nm in names[:8]] + names[:8] + names[-3:]
    return q


def texts():
    """name -> (text, rec_pos)"""
    rng = random.Random("name_sets:texts")
    seq = lambda: acgt(rng, rng.randint(1, 70))
    d = {}
    # ---- names of every length of LENGTHS: once alone, once more with a comment, once with another last byte ----
    for kind, rec in (("fa", fa), ("fq", fq)):
        recs = []
        for n in LENGTHS:
            nm = rand_name(rng, n)
            recs += [rec(nm, seq()), rec(nm + b" a comment", seq())]
            if n:
                recs.append(rec(nm[:-1] + other(nm[-1:]), seq()))
        rng.shuffle(recs)
        d["lengths_" + kind] = build(recs)
    # ---- prefixes of one another, in both orders ----
    pre = [b"read1", b"read10", b"read100", b"read", b"rea", b"read10", b"read1", b"r"]
    d["prefixes"] = build([fa(nm, seq()) for nm in pre] + [fq(nm + b"/2", seq()) for nm in reversed(pre)])
    long_ = rand_name(rng, 300)
    d["long_prefixes"] = build([fa(long_[:k], seq()) for k in (300, 299, 261, 260, 259, 256, 4, 300, 260)])
    # ---- bytes >= 0x80 and NUL ----
    high = [b"n\x80m", b"n\x81m", b"n\xffm", b"\xff\xfe\xfd\xfc\xfb", b"n\x00m", b"n\x00", b"n", b"\x00", b"\x80" * 260, b"\x80" * 259 + b"\x81", b"n\x80m"]
    d["high_bytes"] = build([fa(nm, seq()) for nm in high])
    # ---- what cuts a name: tab, space, '\r', '\n', vertical tab, form feed; 0x0E and 0x1F do not ----
    cuts = [b"x\ty", b"x y", b"x\x0by", b"x\x0cy", b"xy", b"x\x0ey", b"x\x1fy z", b"cut", b"cut\ttab", b"cut more"]
    d["cuts"] = build([fa(nm, seq()) for nm in cuts] + [fa(b"crlf", seq(), eol=b"\r\n"), fa(b"crlf2 c", seq(), eol=b"\r\n"), fa(b"", seq()), fa(b" only a comment", seq())])
    # ---- repeated names: the smallest index wins ----
    reps = [b"a", b"b", b"a", b"c", b"b", b"a", b"dd", b"dd", b"c"] * 5
    d["repeats"] = build([fa(nm + (b" %d" % i if i % 2 else b""), seq()) for i, nm in enumerate(reps)])
    # ---- the last header line ends the text without '\n': short, at the lane / wave edge, and a repeat of an earlier name ----
    d["tail_short"] = build([fa(b"first", seq()), fa(b"tail", seq()), b">tail"])
    edge = rand_name(rng, 260)
    d["tail_260"] = build([fa(edge[:259], seq()), fa(b"mid", seq()), b">" + edge])
    d["tail_only"] = build([b">lonely"])
    d["tail_empty_name"] = build([fa(b"q", seq()), b">"])
    return d


def chain(n, seed=0):
    """n records with short distinct names and a few repeats of them: a table of few slots (hash bits cut: one chain that wraps)"""
    rng = random.Random("name_sets:chain:%d:%d" % (n, seed))
    names = []
    while len(names) < n:
        nm = rand_name(rng, rng.choice((1, 2, 3, 4, 5, 7, 8, 9, 12, 17)))
        if nm not in names or rng.random() < 0.1:
            names.append(nm)
    return build([fa(nm, acgt(rng, rng.randint(1, 20))) for nm in names])


def concat(items):
    off = np.zeros(len(items) + 1, np.uint64)
    if items:
        off[1:] = np.cumsum([len(s) for s in items], dtype=np.uint64)
    buf = np.frombuffer(b"".join(items), dtype=np.uint8).copy() if items else np.zeros(0, np.uint8)
    return buf, off
