"""Oracle leaf functions vs the *compiled reference sources* (oracle/_ref, built by
oracle/Makefile where the reference is present: PatternMatcher.cpp, StringCheck.cpp, kseq.cpp,
aho-corasick/*.c).  The reference's answers on these inputs are recorded in tests/golden (tests/refvec.py);
where oracle/_ref is built the recording is checked against the live library as well."""
import ctypes as C
import hashlib
import os
import random
import struct

import pytest

from tests import orc, fastx, refvec

DATA = os.path.join(os.path.dirname(__file__), "golden", "data")


def rs(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def bmp_cases():
    rng = random.Random(1)
    cases = []
    for _ in range(20000):
        alpha = rng.choice([b"ACGT", b"AC", b"ACGTN"])
        t = rs(rng, rng.randint(0, 60), alpha)
        p = rs(rng, rng.randint(0, 10), alpha)
        cases.append((t, p))
    return cases


def bmp_live(cases):
    return [orc.ref().ref_bmp_search(t, len(t), p, len(p)) for t, p in cases]


def test_bmp_search_random_and_edges():
    L = orc.lib()
    cases = bmp_cases()
    want = refvec.answers("bmp_search", cases, bmp_live)
    for (t, p), b in zip(cases, want):
        a = L.orc_bmp_search(t, len(t), p, len(p))
        assert a == b, (t, p)
        if p and len(p) <= len(t):
            assert a == t.find(p)


def levenshtein_cases():
    rng = random.Random(2)
    pairs = [(b"ABCDEF", b"ABDCEF"), (b"ABCDEF", b"BACDEF"), (b"", b"ACGT"), (b"AC", b"ACGT"),
             (b"ACG", b"ACG"), (b"A" * 50, b"A" * 41 + b"C" * 9)]
    for _ in range(3000):
        n, m = rng.randint(0, 70), rng.randint(0, 70)
        s = rs(rng, n)
        if rng.random() < 0.5 and n:
            # mutated copy: exercises the transposition term
            t = bytearray(s)
            for _k in range(rng.randint(0, 6)):
                if len(t) > 2:
                    i = rng.randrange(len(t) - 1)
                    op = rng.random()
                    if op < 0.4:
                        t[i], t[i + 1] = t[i + 1], t[i]
                    elif op < 0.7:
                        del t[i]
                    else:
                        t.insert(i, rng.choice(b"ACGT"))
            t = bytes(t)
        else:
            t = rs(rng, m)
        pairs.append((s, t))
    return pairs


def levenshtein_live(pairs):
    R = orc.ref()
    # the similarity as the bits of the float the reference returns
    return [(R.ref_levenshtein(s, len(s), t, len(t)), struct.unpack("<I", struct.pack("f", R.ref_similarity(s, len(s), t, len(t))))[0])
            for s, t in pairs]


def test_levenshtein_and_similarity():
    L = orc.lib()
    pairs = levenshtein_cases()
    want = refvec.answers("levenshtein_similarity", pairs, levenshtein_live)
    for (s, t), (lev, sim_bits) in zip(pairs, want):
        assert L.orc_levenshtein(s, len(s), t, len(t)) == lev, (s, t)
        a = L.orc_similarity(s, len(s), t, len(t))
        assert struct.pack("f", a) == struct.pack("<I", sim_bits), (s, t, a, sim_bits)
    # documented quirk
    assert L.orc_levenshtein(b"ABCDEF", 6, b"ABDCEF", 6) == 1
    assert L.orc_levenshtein(b"ABCDEF", 6, b"BACDEF", 6) == 2
    # d=9, max=50 -> 0.819999993 (float) which is NOT > 0.82
    s, t = b"A" * 50, b"A" * 41 + b"C" * 9
    assert L.orc_levenshtein(s, 50, t, 50) == 9
    assert float(L.orc_similarity(s, 50, t, 50)) <= 0.82


def first_match_cases():
    """[(patterns, [texts])] of 300 trials"""
    rng = random.Random(3)
    trials = []
    for trial in range(300):
        alpha = rng.choice([b"ACGT", b"AC"])
        base = [rs(rng, rng.randint(4, 14), alpha) for _ in range(rng.randint(1, 6))]
        pats = []
        for b in base:
            pats.append(b)
            # variants: substrings / extensions / duplicates, like DR variant sets
            for _ in range(rng.randint(0, 4)):
                i = rng.randint(0, len(b) - 2)
                j = rng.randint(i + 2, len(b))
                pats.append(rs(rng, rng.randint(0, 2), alpha) + b[i:j] + rs(rng, rng.randint(0, 2), alpha))
        if rng.random() < 0.3:
            pats.append(pats[0])
        texts = []
        for _ in range(60):
            txt = bytearray(rs(rng, rng.randint(0, 80), alpha + (b"N" if rng.random() < 0.3 else b"")))
            if rng.random() < 0.7 and len(txt) > 20:
                p = rng.choice(pats)
                k = rng.randint(0, len(txt) - 1)
                txt[k:k] = p
            texts.append(bytes(txt))
        trials.append((pats, texts))
    return trials


def first_match_live(trials):
    out = []
    for pats, texts in trials:
        R = orc.PatternSet(pats, "ref")
        out.append([R.first(txt) for txt in texts])
        R.close()
    return out


def test_first_match_semantics_vs_acism():
    trials = first_match_cases()
    want = refvec.answers("first_match_acism", trials, first_match_live)
    for (pats, texts), want_t in zip(trials, want):
        A = orc.PatternSet(pats, "oracle")
        for txt, b in zip(texts, want_t):
            a = A.first(txt)
            assert refvec.plain(a) == b, (pats, txt, a, b)
            if a is not None:
                e, l = a
                # min end position, ties -> longest
                ends = [(i + len(p), -len(p)) for p in set(pats) for i in range(len(txt) - len(p) + 1)
                        if txt[i:i + len(p)] == p]
                assert (e, -l) == min(ends)
        A.close()


def stringcheck_cases():
    rng = random.Random(4)
    pool = [rs(rng, rng.randint(23, 47)) for _ in range(50)]
    return [rng.choice(pool) for _ in range(500)]


def stringcheck_live(seq):
    arr, lens = orc._strarr(seq)
    out = (C.c_int32 * len(seq))()
    orc.ref().ref_stringcheck_tokens(arr, lens, len(seq), out)
    return list(out)


def test_stringcheck_tokens():
    seq = stringcheck_cases()
    out = refvec.answers("stringcheck_tokens", seq, stringcheck_live)
    # oracle/host rule: first token 2, discovery order
    seen = {}
    for s, t in zip(seq, out):
        if s not in seen:
            seen[s] = len(seen) + 2
        assert seen[s] == t


def _dump(recs):
    """records in ref_kseq_dump's layout: per record 4 fields, each <u32 length> + bytes, 0xFFFFFFFF for none"""
    out = bytearray()
    for rec in recs:
        for f in rec:
            if f is None:
                out += struct.pack("<I", 0xFFFFFFFF)
            else:
                out += struct.pack("<I", len(f)) + f
    return bytes(out)


def kseq_case(fname):
    with open(os.path.join(DATA, fname), "rb") as fh:
        return [fname, hashlib.sha256(fh.read()).hexdigest()]


def kseq_live(case):
    path = os.path.join(DATA, case[0])
    out = C.POINTER(C.c_ubyte)()
    ol = C.c_size_t()
    lr = C.c_int()
    n = orc.ref().ref_kseq_dump(path.encode(), C.byref(out), C.byref(ol), C.byref(lr))
    raw = C.string_at(out, ol.value)
    orc.ref().ref_free(out)
    return [n, hashlib.sha256(raw).hexdigest()]


@pytest.mark.parametrize("fname", sorted(os.listdir(DATA)))
def test_python_fastx_reader_matches_kseq(fname):
    n, raw_sha = refvec.answers("kseq_dump/" + fname, kseq_case(fname), kseq_live)
    recs = fastx.read_fastx(os.path.join(DATA, fname))
    assert len(recs) == n
    assert hashlib.sha256(_dump(recs)).hexdigest() == raw_sha


# what tests/golden/make_ref_vectors.py records: name -> (inputs, live reference)
RECORDS = {"bmp_search": (bmp_cases, bmp_live), "levenshtein_similarity": (levenshtein_cases, levenshtein_live),
           "first_match_acism": (first_match_cases, first_match_live), "stringcheck_tokens": (stringcheck_cases, stringcheck_live)}
RECORDS.update({"kseq_dump/" + f: ((lambda f=f: kseq_case(f)), kseq_live) for f in sorted(os.listdir(DATA))})
