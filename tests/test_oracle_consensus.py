"""The oracle of the stage behind the hot path (findConsensusDRs — true-DR consensus, group
splitting, start/stop repair):
* its ksw_align restatement against the COMPILED reference ksw.c (oracle/_ref), with the scoring the Aligner uses, on both
  orientations of every query and on queries up to k_cons_ksw's 320 codes, and its smithWaterman restatement against the
  COMPILED SmithWaterman.cpp (the reference's answers recorded in tests/golden, tests/refvec.py; checked against the live
  library where it is built; the same records pin the device kernels in tests/test_gpu_consensus_kernels.py);
* the whole stage against the known answers SURVEY §8c recorded from the compiled reference: true DR strings, group ids
  and per-group read counts on the reference's own regression inputs."""
import os
import random

import numpy as np
import pytest

from tests import orc, fastx, refvec

DATA = os.path.join(os.path.dirname(__file__), "golden", "data")


def ksw_cases():
    rng = random.Random(11)
    cases = []
    for case in range(6000):
        tl = rng.randint(1, 60)
        t = [rng.randrange(4) for _ in range(tl)]
        kind = rng.random()
        if kind < 0.5:                      # a mutated piece of the target (the DR-variant case)
            a, b = sorted((rng.randrange(tl + 1), rng.randrange(tl + 1)))
            q = t[a:b] or [rng.randrange(4)]
            for _ in range(rng.choice([0, 0, 1, 2, 3])):
                op = rng.random()
                pos = rng.randrange(len(q))
                if op < 0.5:
                    q[pos] = rng.randrange(5)               # 4 = ambiguous base
                elif op < 0.75 and len(q) > 1:
                    del q[pos]
                else:
                    q.insert(pos, rng.randrange(4))
            if rng.random() < 0.3:
                q = [rng.randrange(4) for _ in range(rng.randint(0, 4))] + q + [rng.randrange(4) for _ in range(rng.randint(0, 4))]
        elif kind < 0.8:
            q = [rng.randrange(5) for _ in range(rng.randint(1, 60))]
        else:                                # low-complexity: ties everywhere
            q = [rng.choice([0, 0, 0, 1]) for _ in range(rng.randint(1, 40))]
            t = [rng.choice([0, 0, 0, 1]) for _ in range(tl)]
        cases.append((q, t))
    return cases


def ksw_live(cases):
    if not hasattr(orc.ref(), "ref_ksw_align"):
        return None
    return [orc.ksw_align(q, t, "ref") for q, t in cases]


def revcomp_codes(q):
    """codes 0..3 complemented (3 - c) and reversed, 4 stays 4: the second string k_cons_ksw aligns of every query"""
    return [3 - c if c < 4 else 4 for c in reversed(q)]


def ksw_rc_cases():
    return [(revcomp_codes(q), t) for q, t in ksw_cases()]


KSW_MAX_QLEN = 320                      # k_cons_ksw's LDS cap: 4 x 320 int16 x 64 threads = 160 KB
KSW_MAX_TLEN = 240                      # CRASS_HIP_MAX_DR


def ksw_long_cases():
    """queries of 61..320 codes (the striped layout has slen = ceil(qlen / 8) vectors: lengths near multiples of 8 and at the
    64 / 128 / 240 / 320 steps weighted), targets up to 240"""
    rng = random.Random(12)
    steps = [64, 65, 128, 129, 240, 320]
    cases = []
    for case in range(2000):
        u = rng.random()
        if u < 0.3:
            ql = rng.choice(steps)
        elif u < 0.7:
            ql = min(KSW_MAX_QLEN, max(61, 8 * rng.randint(8, 40) + rng.choice([-1, 0, 1])))
        else:
            ql = rng.randint(61, KSW_MAX_QLEN)
        tl = rng.randint(1, KSW_MAX_TLEN)
        kind = rng.random()
        if kind < 0.5:                      # a mutated piece of the target, padded up to the query length
            t = [rng.randrange(4) for _ in range(tl)]
            a = rng.randrange(tl)
            q = t[a:a + ql]
            for _ in range(rng.choice([0, 1, 2, 4, 8])):
                pos = rng.randrange(len(q))
                op = rng.random()
                if op < 0.5:
                    q[pos] = rng.randrange(5)
                elif op < 0.75 and len(q) > 1:
                    del q[pos]
                else:
                    q.insert(pos, rng.randrange(4))
            lead = rng.randint(0, max(0, ql - len(q)))
            q = [rng.randrange(4) for _ in range(lead)] + q
            q = (q + [rng.randrange(4) for _ in range(ql - len(q))])[:ql]
        elif kind < 0.8:
            t = [rng.randrange(4) for _ in range(tl)]
            q = [rng.randrange(5) for _ in range(ql)]
        else:                                # low-complexity: ties everywhere
            t = [rng.choice([0, 0, 0, 1]) for _ in range(tl)]
            q = [rng.choice([0, 0, 0, 1]) for _ in range(ql)]
        cases.append((q, t))
    return cases


def test_ksw_align_matches_the_compiled_reference():
    cases = ksw_cases()
    n = 0
    for (q, t), want in zip(cases, refvec.answers("ksw_align", cases, ksw_live)):
        got = orc.ksw_align(q, t, "oracle")
        assert list(got) == want, (q, t, got, want)
        n += want[0] >= 5
    assert n > 2000


def test_ksw_align_reverse_complement_matches_the_compiled_reference():
    cases = ksw_rc_cases()
    for (q, t), want in zip(cases, refvec.answers("ksw_align_rc", cases, ksw_live)):
        assert list(orc.ksw_align(q, t, "oracle")) == want, (q, t, want)


def ksw_long_rc_cases():
    return [(revcomp_codes(q), t) for q, t in ksw_long_cases()]


def test_ksw_align_long_queries_match_the_compiled_reference():
    cases = ksw_long_cases()
    qls = [len(q) for q, _ in cases]
    assert min(qls) == 61 and max(qls) == KSW_MAX_QLEN and all(x in qls for x in (64, 65, 128, 129, 240))
    n = 0
    for (q, t), want in zip(cases, refvec.answers("ksw_align_long", cases, ksw_live)):
        assert list(orc.ksw_align(q, t, "oracle")) == want, (q, t, want)
        n += want[0] >= 5 and want[3] >= 0
    assert n > 500
    cases = ksw_long_rc_cases()
    for (q, t), want in zip(cases, refvec.answers("ksw_align_long_rc", cases, ksw_live)):
        assert list(orc.ksw_align(q, t, "oracle")) == want, (q, t, want)


SW_LDS_DIR, SW_LDS_A = 8192, 256        # consensus_internal.h: k_cons_sw's per-wave LDS (direction bytes, read window)


def sw_form(length, dr_len):
    """which of k_cons_sw's three forms a task takes (cons_sw_in_lds, consensus_internal.h): 0 wavefront with the direction
    matrix in LDS, 1 wavefront with it in global scratch, 2 the serial lane-0 form (DR longer than 64)"""
    if dr_len > 64:
        return 2
    return 0 if (length + 1) * (dr_len + 1) <= SW_LDS_DIR and length <= SW_LDS_A else 1


def sw_cases():
    """(read, DR, start, len, similarity) inside the reference's domain: 0 <= start, 1 <= len, start + len <= len(read)"""
    rng = random.Random(13)
    odd = b"NnacgtRY.-"

    def rnd(n, alpha=b"ACGT"):
        return bytes(rng.choice(alpha) for _ in range(n))

    def mutate(x, k):
        x = bytearray(x)
        for _ in range(k):
            pos = rng.randrange(len(x)) if x else 0
            op = rng.random()
            if op < 0.5 and x:
                x[pos] = rng.choice(b"ACGT")
            elif op < 0.75 and len(x) > 1:
                del x[pos]
            else:
                x.insert(pos, rng.choice(b"ACGT"))
        return bytes(x)

    def dr_len():
        u = rng.random()
        if u < 0.3:
            return rng.choice([63, 64, 65])
        if u < 0.45:
            return rng.randint(1, 8)
        return rng.randint(9, 130)

    cases = []
    for case in range(4000):
        kind = rng.random()
        sim = rng.choice([0.0, 0.85, 0.85])
        if kind < 0.3:                          # partial repeats at both read ends around full copies (updateStartStops)
            dl = dr_len()
            dr = rnd(dl)
            sp = rnd(rng.randint(20, 50))
            head, tail = dr[rng.randint(0, dl - 1):], dr[:rng.randint(1, dl)]
            copies = rng.randint(1, 4)
            body = (dr + sp) * copies
            read = rnd(rng.randint(0, 20)) * (rng.random() < 0.3) + mutate(head, rng.choice([0, 0, 1])) + sp + body + \
                mutate(tail, rng.choice([0, 0, 1]))
            if rng.random() < 0.5:              # front search: [0, first start - lowSpacer)
                start, length = 0, max(1, len(head) + rng.randint(0, len(sp)))
            else:
                start = max(0, len(read) - len(tail) - rng.randint(0, 30))
                length = len(read) - start
        elif kind < 0.45:                       # windows across the LDS / scratch test
            dl = rng.choice([rng.randint(20, 64), 63, 64, 31, 32])
            u = rng.random()
            if u < 0.5:
                length = max(1, SW_LDS_DIR // (dl + 1) - 1 + rng.randint(-2, 2))
            else:
                length = rng.choice([255, 256, 257])
            dr = rnd(dl)
            pre = rnd(rng.randint(0, 40))
            read = pre + rnd(length)
            ins = rng.randrange(max(1, length - dl)) if length > dl else 0
            read = read[:len(pre) + ins] + mutate(dr, rng.randint(0, 3)) + read[len(pre) + ins:]
            start = rng.randint(0, len(pre))
            length = min(length, len(read) - start)
        elif kind < 0.55:                       # long reads, long windows
            dl = dr_len()
            dr = rnd(dl)
            L = rng.randint(300, 2000)
            read = bytearray(rnd(L))
            for _ in range(rng.randint(0, 6)):
                p = rng.randrange(L)
                piece = mutate(dr, rng.randint(0, 3))
                read[p:p + len(piece)] = piece
            read = bytes(read[:L])
            start = rng.choice([0, rng.randrange(L)])
            length = rng.randint(1, L - start)
        elif kind < 0.65:                       # length 1 and 2, start > 0
            dl = dr_len()
            dr = rnd(dl)
            read = rnd(rng.randint(3, 120))
            length = rng.choice([1, 2])
            start = rng.randint(0, len(read) - length)
        elif kind < 0.8:                        # the 0.85 boundary: a piece of 20 / 40 / 60 bases at edit distance 3 / 6 / 9
            m = rng.choice([1, 2, 3])
            dl = rng.randint(20 * m, min(130, 20 * m + 30))
            dr = rnd(dl)
            a = rng.randint(0, dl - 20 * m)
            piece = bytearray(dr[a:a + 20 * m])
            for p in rng.sample(range(1, 20 * m - 1), 3 * m):
                piece[p] = rng.choice([c for c in b"ACGT" if c != piece[p]])
            read = rnd(rng.randint(0, 30)) + bytes(piece) + rnd(rng.randint(0, 30))
            start, length = 0, len(read)
            sim = 0.85
        elif kind < 0.9:                        # low complexity: score ties everywhere
            dl = dr_len()
            dr = rnd(dl, b"AAAT")
            read = rnd(rng.randint(1, 300), rng.choice([b"AAAT", b"AT", b"A"]))
            start = rng.randrange(len(read))
            length = rng.randint(1, len(read) - start)
        else:                                   # N, lowercase and other bytes (never equal to a DR base unless identical)
            dl = dr_len()
            dr = rnd(dl, b"ACGTACGTNa")
            read = rnd(rng.randint(1, 300), b"ACGTACGT" + odd)
            read = read[:rng.randrange(len(read) + 1)] + mutate(dr, 1) + read[len(read) // 2:]
            start = rng.randrange(len(read))
            length = rng.randint(1, len(read) - start)
        assert 0 <= start and 1 <= length and start + length <= len(read) and len(dr) >= 1
        cases.append((read, dr, start, length, sim))
    return cases


def sw_live(cases):
    if not hasattr(orc.ref(), "ref_smith_waterman"):
        return None
    return [sw_fields(orc.smith_waterman(a, b, s, n, sim, "ref")) for a, b, s, n, sim in cases]


def sw_fields(r):
    """(ret, aStart, aEnd, a_ret, b_ret) -> JSON-friendly (ret, aStart, aEnd, a_ret, b_ret as text)"""
    ret, s, e, a, b = r
    return [ret, s, e, a.decode("latin-1"), b.decode("latin-1")]


def test_smith_waterman_matches_the_compiled_reference():
    cases = sw_cases()
    forms = [0, 0, 0]
    for c in cases:
        forms[sw_form(c[3], len(c[1]))] += 1
    assert min(forms) >= 100, forms
    want = refvec.answers("smith_waterman", cases, sw_live)
    kinds = {0: 0, 1: 0}
    for (a, b, s, n, sim), w in zip(cases, want):
        got = sw_fields(orc.smith_waterman(a, b, s, n, sim))
        assert got == w, (a, b, s, n, sim, got, w)
        kinds[w[0]] += 1
    assert kinds[0] >= 200 and kinds[1] >= 2000, kinds


def test_smith_waterman_basics():
    dr = b"GTTTCAATCCACGCGCCCACGCGGGGCGCGAC"
    read = b"TTATTATATTATTTATATATTATTATAT" + dr[-12:]        # the END of a repeat at the read end: found, but it is no repeat start
    r, s, e, a, b = orc.smith_waterman(read, dr, 10, len(read) - 10)
    # (the traceback also takes in the zero-score cell in front of the local alignment: SmithWaterman.cpp:246-262)
    assert r == 1 and e == len(read) - 1 and a == read[-15:] and b == dr[-15:] and dr.find(b) != 0
    read2 = b"ACGTTGCAGGATCTTACGATCGGATCAG" + dr[:14]       # a repeat START at the read end: the case updateStartStops adds
    r, s, e, a, b = orc.smith_waterman(read2, dr, 10, len(read2) - 10)
    assert r == 1 and (s, e) == (28, len(read2) - 1) and a == b == dr[:14] and dr.find(b) == 0
    # the reference cuts a_ret with a length that includes aStartSearch (SmithWaterman.cpp:279): with a search window that
    # starts inside the read, a_ret runs on to the end of the read and the similarity is taken over that longer string
    read3 = b"TTATTATATTATTTATATATTATTATAT" + dr[:14] + b"TTATATTAT"
    r0, s0, e0, a0, b0 = orc.smith_waterman(read3, dr, 10, len(read3) - 10, 0.0)
    assert r0 == 1 and (s0, e0) == (28, 41) and a0 == read3[28:] and b0 == dr[:14]
    assert orc.smith_waterman(read3, dr, 10, len(read3) - 10) == (0, 0, 0, b"", b"")     # not similar enough: ("", "") and zeros


# file: (true DRs by GID, reads per group)  — SURVEY.md §8c
KNOWN = {
    "Ill100.fx.gz": ({1: b"CGGTTCATCCCCGCGCCTGCGGGGAACGC"}, {1: 4312}),
    "CN_gDC.fa.gz": ({1: b"CTTTTAATCGCACCTATTTGGAATTGAAAC"}, None),
    "front_offset_bug.fa.gz": ({10: b"CGCTCTGGCCGGTCTCCGACCGAGCCAGCCC", 20: None, 44: None, 45: None}, {10: 303, 20: 102, 44: 35, 45: 28}),
}


@pytest.mark.parametrize("fname", sorted(KNOWN))
def test_true_dr_known_answers(fname):
    recs = fastx.read_fastx(os.path.join(DATA, fname))
    seqs, hdrs = [r[2] for r in recs], [r[0] for r in recs]
    res = orc.pipeline(seqs, hdrs)
    con = orc.consensus(seqs, res)
    assert con.error == 0
    drs, counts = KNOWN[fname]
    assert con.gids == sorted(drs)
    for gid, dr, n_reads in zip(con.gids, con.true_drs, con.group_read_counts()):
        if drs[gid] is not None:
            assert dr == drs[gid]
        if counts is not None:
            assert n_reads == counts[gid]
        assert dr <= orc_revcomp(dr)                           # laurenized
    # structural invariants of the repaired records
    for k in range(len(con.rec_alive)):
        if con.rec_alive[k] and con.rec_token[k]:
            ss = con.ss(k)
            assert len(ss) % 2 == 0 and ss == sorted(ss)


def orc_revcomp(s):
    import ctypes as C
    out = C.create_string_buffer(len(s))
    orc.lib().orc_revcomp(s, len(s), out)
    return out.raw


@pytest.mark.parametrize("fname", ["Ill.nr.miss.fa.gz", "poor_dr_ext.fa.gz"])
def test_other_reference_inputs_run_clean(fname):
    recs = fastx.read_fastx(os.path.join(DATA, fname))
    seqs, hdrs = [r[2] for r in recs], [r[0] for r in recs]
    con = orc.consensus(seqs, orc.pipeline(seqs, hdrs))
    assert con.error == 0 and len(con.gids) >= 1


class WithGap:
    """a search result whose mDR2GIDMap has a NULL entry at GID 1 (every original group moves up by one)"""

    def __init__(self, res):
        self.__dict__.update(res.__dict__)
        self.groups = [[]] + [list(g) for g in res.groups]


def test_a_gid_without_a_group_is_skipped():
    """WorkHorse::findConsensusDRs `continue`s over a NULL group (WorkHorse.cpp:592-595): same true DRs one GID higher"""
    recs = fastx.read_fastx(os.path.join(DATA, "front_offset_bug.fa.gz"))
    seqs, hdrs = [r[2] for r in recs], [r[0] for r in recs]
    res = orc.pipeline(seqs, hdrs)
    a, b = orc.consensus(seqs, res), orc.consensus(seqs, WithGap(res))
    assert a.error == 0 and b.error == 0
    assert b.gids == [g + 1 for g in a.gids] and b.true_drs == a.true_drs and b.groups == a.groups
    assert b.next_free_gid == a.next_free_gid + 1


# what tests/golden/make_ref_vectors.py records: name -> (inputs, live reference)
RECORDS = {"ksw_align": (ksw_cases, ksw_live), "ksw_align_rc": (ksw_rc_cases, ksw_live),
           "ksw_align_long": (ksw_long_cases, ksw_live), "ksw_align_long_rc": (ksw_long_rc_cases, ksw_live),
           "smith_waterman": (sw_cases, sw_live)}
