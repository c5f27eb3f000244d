"""Designed reads for the lane kernel's stages behind its seed find (k_survivor_lanes, crass_amd/csrc/survivor_lanes.hip): the
pooled QC (qc_pool_begin_queued, qc_enqueue_above, qc_run_task, qc_pool_end, ln_lev_regs' early stop), the extension (ln_extend2,
ln_extend) and the inline DRLowLexi.  CPU only, seeded, deterministic.  tests/test_lane_sets_host.py pins the design on the
oracle; tests/test_gpu_lane_sets.py runs the sets through the kernels.

Every edge is a TWIN PAIR (Pair): two reads one step apart across the edge, each with the answer written down from its design
(found or not, replen, low-lexi flag, start/stops).  A pair is kept only if orc.search_core gives exactly both designed answers
and the two answers differ; `why` holds the component values that explain the flip (edit distances, similarities, the
low-complexity verdict, the QC verdict on the designed start/stops), which the host test checks side by side.

Backgrounds are clean (walk_sets.clean: no w-mer stands again D0 .. D1 further on), the array's flank columns are set so that
no column next to a repeat passes a vote unless the design says so (the flank control of test_gpu_lane_find._repeats, here by
the spacers' own first and last bases and the bases in front of and behind the array).

Kinds (the sub-case is in Pair.sub):
  sim2            two repeats, repeat against spacer at the cut: the spacer is the repeat with edits (plus a random tail), n the
                  repeat's length, m the spacer length the QC measures (one base short), d_no(max(n, m)) the smallest distance
                  whose similarity is not above 0.82, by the reference's own float expression.  Distance d_no - 1 (rejected)
                  | d_no (found), the twins ONE BASE apart.  Edits spread out, all in the first columns (the early stop fires
                  at once), all in the last (the loop runs to its end)
  transposition   distance d_no - 1 only if an adjacent swap counts as one edit: the swap at bases 0-1 (the reference's i, j > 2
                  counts two: found) | at 1-2 or at the last pair (one: rejected)
  sim3            three repeats: spacer against spacer at the cut (ss), repeat against first spacer at the cut with the first
                  test far below (rs), and both tests at the cut, the first | the second one deciding (both_a, both_b)
  words           the shorter string of 31, 32, 33 bases (32-bit task, 32-bit task, 64-bit task), n == m; under -D 64 -S 70
                  63 and 64 against 64 (bit 63, the full mask)
  lengths         two repeats: measured spacer lowSp - 1 | lowSp, highSp | highSp + 1; three: the shorter spacer, the longer,
                  |s1 - s2| 12 | 13; |repeat - spacer| 30 | 31 for two and three repeats under -s 20 -S 60
  low_complexity  repeats holding int(0.75 len) | that + 1 copies of one letter, each of A, C, G, T
  extend2         repeat of lowDR - 1 | lowDR and highDR | highDR + 1 from seed offset 0, 4 and 7 (right only, both, mostly left) and
                  from the LAST offset behind a lead decoy; first repeat at base 0 | 1 | 2; second repeat ending at L - 1 | L - 2;
                  under -D 75 right and left runs of 63 | 64 | 65 columns (the second 64-base chunk) and 75 | 76 bases
  votes           3, 4, 5, 7 repeats: a flank column in which max(2, n - 1) - 1 | max(2, n - 1) copies agree, left and right, per
                  letter; the last repeat cut by the read's end; the first repeat at base 0; the shortest spacing not the first
  chain           four repeats, spacers a, a +- 24, a | a, a +- 25, a (walk_sets' third kind under the defaults: the twin keeps two)
  orientation     the repeat's first difference from its reverse complement at base 0, 15, 16, 31, 32 and the last possible one,
                  lower and higher; palindromes; the first repeat at base 0.  THE TWIN IS THE READ'S REVERSE COMPLEMENT: the same
                  DR string, the other flag, mirrored start/stops.  Lengths 23 .. 47 (both 128-bit `drop` cases below 64), 64
                  (drop 0) and 65 .. 75 (the byte loop) under -D 75
  second_round    the first candidate rejected by a pooled test (a sim2 twin at d_no - 1) or by its spacer's length, a real array
                  behind it | the same read with the first candidate accepted: the first array is the record
  field_edges     sim2 twins whose array ends at L - 1 and L - 2 of reads of 512, 511 and 497 bases: s0 / t0 at the top of 9 bits
  pool            (full_pool) three-repeat arrays only, repeat lengths alternating about 32: every lane queues two tests

LEFT OUT, with the reason:
  extend2's right run ended by spacing - lowSp, its left run ended by spacing - len_r, and votes' caps likewise: a run that
      reaches the cap leaves a spacer of lowSp - w - left (right) or of 0 bases (left) — qcFoundRepeats rejects it, and the next
      seed is taken from the last STOP, which no left run moves.  No record can depend on either cap.
  the pick rule's lenA > lenB: with two repeats both copies get the same two runs and neither clamp of the start/stops binds (the
      right run ends before the second copy's column leaves the read, the left run at the first copy's base 0), so the
      lengths are equal and the pick is the second repeat — always.  Reads with the first repeat at base 0 are in.
  chain's `repeat_spacing < lowSp + w`: scanRight's window begins at last + w + lowSp, so a found copy is never nearer.
  a transposition in the cells i = 2 or j = 2 alone (the restriction i, j > 2 taken one index at a time): it cannot lower a
      distance.  The term offers M[i-2][0] + 1 = i - 1 for cell (i, 2), and the plain recurrence reaches i - 1 there already
      (substitute t1 for s[i-2], match t2 = s[i-1], delete the rest).  Only cell (2, 2) gains, which is the swap at bases 0-1.
  the early stop of ln_lev_regs written one column LATE stops later and returns the same distances; see the GPU module.

By design no read is handed to the wave kernel: every compared string has at most 64 bases (but the repeats of 65 .. 76 bases
under -D 75, which ln_qc takes in the lane against spacers of 64 bases or fewer: only a pair BOTH beyond 64 is handed over) and
every start/stop list is far below the capacity.  The library reports no counter for the hand-over, so this claim rests on the
code (qc_pool_begin_queued, ln_distance, ln_add), not on an assertion; test_lane_sets_host.py asserts the lengths.
"""
import ctypes as C
import functools

import numpy as np

from tests import orc
from tests import edge_reads as E
from tests import walk_sets as W

DRAWS = {
    "defaults": {},
    "S20_60": dict(lowSpacerSize=20, highSpacerSize=60),
    "D64S70": dict(highDRsize=64, highSpacerSize=70),
    "D75": dict(highDRsize=75),
}
MODES = ("spread", "first", "last")
SIM2_N = (23, 24, 31, 32, 33, 34, 40, 47)
LETTERS = b"ACGT"


def params(draw):
    return orc.Params.default(**DRAWS[draw])


def lev(a, b):
    return orc.lib().orc_levenshtein(a, len(a), b, len(b))


def sim(a, b):
    return float(orc.lib().orc_similarity(a, len(a), b, len(b)))


def low_complexity(s):
    return int(orc.lib().orc_is_low_complexity(s, len(s)))


def qc(seq, spans, p):
    ss = [x for sp in spans for x in sp]
    arr = (C.c_uint32 * len(ss))(*ss)
    return int(orc.lib().orc_qc_found_repeats(seq, len(seq), arr, len(ss), int(p.lowSpacerSize), int(p.highSpacerSize)))


def extend(seq, seeds, p):
    """orc_extend_pre_repeat on seed spans [(start, start + w - 1)] -> (replen, spans)"""
    ss = [x for sp in seeds for x in sp]
    arr = (C.c_uint32 * len(ss))(*ss)
    rl = int(orc.lib().orc_extend_pre_repeat(seq, len(seq), arr, len(ss), int(p.searchWindowLength), int(p.lowSpacerSize)))
    return rl, [(arr[i], arr[i + 1]) for i in range(0, len(ss), 2)]


def d_no(mx):
    """the smallest distance whose similarity over max_length = mx is NOT above 0.82 (qc_enqueue_above's own loop)"""
    d = 0
    while d <= mx and float(np.float32(1.0 - float(np.float32(d) / np.float32(mx)))) > 0.82:
        d += 1
    return d


def osa_free(a, b):
    """the optimal-string-alignment distance with the transposition term in every cell (no i, j > 2)"""
    n, m = len(a), len(b)
    M = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        M[i][0] = i
    for j in range(m + 1):
        M[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            c = min(M[i - 1][j] + 1, M[i][j - 1] + 1, M[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                c = min(c, M[i - 2][j - 2] + 1)
            M[i][j] = c
    return M[n][m]


class Pair:
    """a, b: walk_sets.Read (a: the twin on the near side of the edge); why: the component values that explain the flip"""

    def __init__(self, kind, sub, draw, a, b, why=None):
        self.kind, self.sub, self.draw, self.a, self.b, self.why = kind, sub, draw, a, b, why or {}
        for r in (a, b):
            r.kind, r.sub, r.draw = kind, sub, draw

    @property
    def L(self):
        return self.a.L

    @property
    def name(self):
        return "%s/%s/%s/L%d" % (self.kind, self.sub, self.draw, self.L)


def kept(pairs):
    out = []
    for pr in pairs:
        p = params(pr.draw)
        if pr.a.want() != pr.b.want() and all(W.oracle_record(r, p) == r.want() for r in (pr.a, pr.b)):
            out.append(pr)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# building reads
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bg_pool(pkey, L, n=192):
    p = orc.Params(*pkey)
    return W.background(np.random.default_rng([77, L] + list(pkey)), p, L, n)


class Designer:
    def __init__(self, draw, seed):
        self.draw, self.p = draw, params(draw)
        self.rng = np.random.default_rng([seed] + list(E.key(self.p)))
        self.n_bg = 0

    def bg(self, L):
        pool = _bg_pool(E.key(self.p), L)
        self.n_bg += 1
        return pool[(self.n_bg * 7) % len(pool)].copy()

    def rand(self, n):
        return E._rand(self.rng, n).tobytes()

    def other(self, *not_these):
        c = [x for x in LETTERS if x not in not_these]
        return bytes([c[int(self.rng.integers(0, len(c)))]]) if c else b"A"

    def dr(self, n, flipped=None):
        return W.random_dr(self.rng, n, int(self.p.searchWindowLength), flipped)

    def spacer(self, n, k):
        """a random spacer whose first and last base cycle with k, so that no flank column gets two votes (up to four copies)"""
        s = bytearray(self.rand(n))
        s[0], s[-1] = LETTERS[k % 4], LETTERS[(k + 1) % 4]
        s[1], s[-2] = LETTERS[(k + 2) % 4], LETTERS[(k + 3) % 4]
        return bytes(s)

    def put(self, a, keep, at, copies, spacers, pre=None, post=None):
        """copies[0] spacers[0] copies[1] ... from base `at` of a (in place), pre in front and post behind (default: a base that
        no spacer ends / begins with) -> the copies' spans"""
        body, spans, q = b"", [], at
        for k, c in enumerate(copies):
            spans.append((q, q + len(c) - 1))
            body += c
            q += len(c)
            if k < len(spacers):
                body += spacers[k]
                q += len(spacers[k])
        L = len(a)
        end = at + len(body)
        assert at >= 0 and end <= L + 0, (at, end, L)
        a[at:end] = np.frombuffer(body, np.uint8)
        if pre is None:
            pre = self.other(*[s[-1] for s in spacers])
        if post is None:
            post = self.other(*[s[0] for s in spacers])
        pre, post = pre[-at:] if at else b"", post[:L - end]
        if pre:
            a[at - len(pre):at] = np.frombuffer(pre, np.uint8)
        if post:
            a[end:end + len(post)] = np.frombuffer(post, np.uint8)
        keep[max(0, at - len(pre) - 1):min(L, end + len(post) + 1)] = True
        return spans

    def finish(self, a, keep):
        W.clean(a.reshape(1, -1), self.p, self.rng, keep.reshape(1, -1))
        return a.tobytes()

    def array(self, L, at, copies, spacers, pre=None, post=None):
        a, keep = self.bg(L), np.zeros(L, bool)
        spans = self.put(a, keep, at, copies, spacers, pre, post)
        return self.finish(a, keep), spans

    def read(self, seq, spans=None, found=True, replen=None, **info):
        """the Read of seq with the designed answer: the array `spans` (found) or nothing"""
        info = dict(info, spans=spans)
        if not found:
            return W.Read(seq, "", "", self.draw, False, info=info)
        rl, low, ss = W.answer(seq, spans, replen)
        return W.Read(seq, "", "", self.draw, True, rl, low, ss, info=info)


def patched(seq, at, s):
    return seq[:at] + s + seq[at + len(s):]


def near_twins(D, src, m, dist, mode, must=()):
    """two strings of m bases ONE BASE apart, at distance dist - 1 and dist from src: src cut to m bases or with a random tail, and
    substitutions one by one — evenly spread, from the first column on, or from the last column of the shorter string down.
    must: positions substituted first.  None where the lengths alone are further apart than dist - 1."""
    n = len(src)
    k = min(n, m)
    for _ in range(80):
        cur = src[:m] if m <= n else src + D.rand(m - n)
        if lev(src, cur) > dist - 1:
            if m <= n:
                return None
            continue
        if mode == "first":
            order = list(range(k))
        elif mode == "last":
            order = list(range(k - 1, -1, -1))
        else:
            order = [int((i + 0.5) * k / dist) for i in range(dist)]
            order += [int(x) for x in D.rng.permutation(k) if int(x) not in order]
        order = list(must) + [q for q in order if q not in must]
        for i, q in enumerate(order):
            nxt = bytearray(cur)
            nxt[q] = D.other(cur[q], src[q] if q < n else 0)[0]
            nxt = bytes(nxt)
            d = lev(src, nxt)
            if d >= dist:
                if d == dist and i >= len(must) and lev(src, cur) == dist - 1:
                    return cur, nxt
                break
            cur = nxt
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the kinds
# ---------------------------------------------------------------------------------------------------------------------
def _m_choices(p, n):
    lo, hi = int(p.lowSpacerSize), int(p.highSpacerSize)
    ms = [m for m in (n - 2, n, n + 2) if lo <= m <= hi]
    return ms if len(ms) == 3 else [m for m in (lo, lo + 1, n + 2) if m <= hi]


def _sim2_pair(D, kind, sub, L, n, m, mode, at=None, end_at=None, behind=None):
    """one sim2 twin pair: the array at `at`, or ending with base end_at; behind: (DR length, spacer length) of a real array
    placed after it (second_round: the found twin's record is the first array, the rejected twin's the second)"""
    dn = d_no(max(n, m))
    dr = D.dr(n)
    tw = near_twins(D, dr, m, dn, mode)
    if tw is None:
        return None
    tail = D.other(dr[0])                                           # the spacer's last base, which the QC does not measure
    span = 2 * n + m + 1
    if at is None:
        at = end_at + 1 - span
    if at < 0 or at + span > L:
        return None
    a, keep = D.bg(L), np.zeros(L, bool)
    post = D.other(tw[0][0], tw[1][0])
    spans = D.put(a, keep, at, [dr, dr], [tw[0] + tail], post=post)
    spans2 = None
    if behind:
        n2, sp2 = behind
        at2 = at + span + 10
        if at2 + 2 * n2 + sp2 > L - 1:
            return None
        dr2 = D.dr(n2)
        spans2 = D.put(a, keep, at2, [dr2, dr2], [D.spacer(sp2, 0)])
    seq_a = D.finish(a, keep)
    seq_b = patched(seq_a, at + n, tw[1])
    why = dict(n=n, m=m, d_no=dn, mode=mode, dr=dr, sp=(tw[0], tw[1]), lev=(lev(dr, tw[0]), lev(dr, tw[1])),
               sim=(sim(dr, tw[0]), sim(dr, tw[1])), qc=(qc(seq_a, spans, D.p), qc(seq_b, spans, D.p)))
    ra = D.read(seq_a, spans2, found=True) if behind else D.read(seq_a, spans, found=False)
    return Pair(kind, sub, D.draw, ra, D.read(seq_b, spans), why)


@functools.lru_cache(maxsize=None)
def sim2(draw="defaults", L=150, seed=31, reps=1):
    D = Designer(draw, seed + L)
    out = []
    for rep in range(reps):
        for n in SIM2_N:
            for m in _m_choices(D.p, n):
                for mode in MODES:
                    pr = _sim2_pair(D, "sim2", "n%d_m%d_%s" % (n, m, mode), L, n, m, mode, at=8 * (1 + (len(out) + rep) % 2))
                    if pr:
                        out.append(pr)
    return kept(out)


@functools.lru_cache(maxsize=None)
def words(draw="defaults", L=150, seed=32):
    D = Designer(draw, seed + L)
    cells = [(31, 31), (32, 32), (33, 33)] if draw == "defaults" else [(63, 64), (64, 64)]
    out = []
    for n, m in cells:
        for mode in MODES if draw == "defaults" else ("spread", "spread", "spread"):
            for _ in range(2):
                pr = _sim2_pair(D, "words", "n%d_m%d" % (n, m), L, n, m, mode, at=8)
                if pr:
                    out.append(pr)
    return kept(out)


TRANSPOSITIONS = ("swap01|swap12", "swap01|swap_last")


@functools.lru_cache(maxsize=None)
def transposition(draw="defaults", L=150, seed=33):
    D = Designer(draw, seed + L)
    out = []
    for n in (32, 33, 40):
        dn = d_no(n)
        for var in TRANSPOSITIONS:
            for _ in range(60):
                dr = D.dr(n)
                if len(set(dr[:2])) < 2 or len(set(dr[1:3])) < 2 or len(set(dr[2:4])) < 2 or dr[-1] == dr[-2]:
                    continue
                sw = lambda s, i: s[:i] + bytes([s[i + 1], s[i]]) + s[i + 2:]
                if var == "swap01|swap12":
                    x, y = sw(dr, 0), sw(dr, 1)
                else:
                    x, y = sw(dr, 0), sw(dr, n - 2)
                ok = False
                for q in [int(v) for v in D.rng.permutation(np.arange(8, n - 6, 3))]:
                    if lev(dr, x) >= dn:
                        break
                    c = D.other(x[q], dr[q], dr[q - 1], dr[q + 1])
                    x, y = patched(x, q, c), patched(y, q, c)
                ok = lev(dr, x) == dn and lev(dr, y) == dn - 1 and osa_free(dr, x) == dn - 1
                if not ok:
                    continue
                tail = D.other(dr[0])
                seq_y, spans = D.array(L, 8, [dr, dr], [y + tail], post=D.other(x[0], y[0]))
                seq_x = patched(seq_y, 8 + n, x)
                why = dict(n=n, m=n, d_no=dn, dr=dr, sp=(y, x), lev=(lev(dr, y), lev(dr, x)), free=(osa_free(dr, y), osa_free(dr, x)),
                           sim=(sim(dr, y), sim(dr, x)), qc=(qc(seq_y, spans, D.p), qc(seq_x, spans, D.p)))
                out.append(Pair("transposition", var, draw, D.read(seq_y, spans, found=False), D.read(seq_x, spans), why))
                break
    return kept(out)


SIM3 = ("ss", "rs", "both_a", "both_b")


@functools.lru_cache(maxsize=None)
def sim3(draw="defaults", L=251, seed=34):
    """three repeats; S1, S2 of the same length m.  a: rejected, b: found"""
    D = Designer(draw, seed + L)
    out = []
    for n in (24, 31, 32, 33, 40):
        m = max(n, 27)
        if 8 + 3 * n + 2 * m + 1 > L:
            continue
        dn, ends = d_no(m), (0, m - 1)
        for sub in SIM3:
            for mode in ("spread", "last"):
                dr = D.dr(n)
                if sub == "ss":
                    s1 = D.spacer(m, 0)
                    tw = near_twins(D, s1, m, dn, mode, must=ends)
                    cand = tw and [(s1, tw[0]), (s1, tw[1])]
                elif sub == "rs":
                    tw = near_twins(D, dr, m, dn, mode)
                    s2 = tw and D.other(tw[0][0], tw[1][0]) + D.rand(m - 2) + D.other(tw[0][-1], tw[1][-1])
                    cand = tw and [(tw[0], s2), (tw[1], s2)]
                elif sub == "both_a":                               # the second test just passes; the first decides
                    t1 = near_twins(D, dr, m, dn, mode)
                    tw = t1 and near_twins(D, t1[1], m, dn, mode, must=ends)
                    cand = tw and [(t1[1], tw[0]), (t1[1], tw[1])]
                else:                                               # the first test just passes; the second decides
                    t1 = near_twins(D, dr, m, dn, mode)
                    tw = t1 and near_twins(D, t1[1], m, dn, mode, must=ends)
                    cand = tw and lev(t1[0], tw[1]) >= dn and [(t1[0], tw[1]), (t1[1], tw[1])]
                if not cand:
                    continue
                (a1, a2), (b1, b2) = cand
                # the three flank columns on either side pairwise different: no column passes a vote (cut_off 2)
                rcol, lcol = {a1[0], a2[0], b1[0], b2[0]}, {a1[-1], a2[-1], b1[-1], b2[-1]}
                if len(rcol) > 3 or len(lcol) > 3 or a1[0] == a2[0] or b1[0] == b2[0] or a1[-1] == a2[-1] or b1[-1] == b2[-1]:
                    continue
                seq_a, spans = D.array(L, 8, [dr] * 3, [a1, a2], pre=D.other(*lcol), post=D.other(*rcol))
                seq_b = patched(patched(seq_a, 8 + n, b1), 8 + 2 * n + m, b2)
                why = dict(n=n, m=m, d_no=dn, mode=mode, dr=dr, a=(a1, a2), b=(b1, b2),
                           lev_ss=(lev(a1, a2), lev(b1, b2)), lev_rs=(lev(dr, a1), lev(dr, b1)),
                           sim_ss=(sim(a1, a2), sim(b1, b2)), sim_rs=(sim(dr, a1), sim(dr, b1)),
                           qc=(qc(seq_a, spans, D.p), qc(seq_b, spans, D.p)))
                out.append(Pair("sim3", "%s_n%d" % (sub, n), draw, D.read(seq_a, spans, found=False), D.read(seq_b, spans), why))
    return kept(out)


def _plain(D, L, n, sps, at=8, found=True, dr=None):
    dr = dr or D.dr(n)
    if at + (len(sps) + 1) * n + sum(sps) > L:
        return None
    seq, spans = D.array(L, at, [dr] * (len(sps) + 1), [D.spacer(s, k) for k, s in enumerate(sps)])
    return D.read(seq, spans, found=found, qc=qc(seq, spans, D.p), sps=list(sps), n=n)


@functools.lru_cache(maxsize=None)
def lengths(draw="defaults", L=251, seed=35):
    """(a | b) one spacer base apart.  The measured spacer of two repeats is one base short"""
    D = Designer(draw, seed + L)
    lo, hi = int(D.p.lowSpacerSize), int(D.p.highSpacerSize)
    plans = []
    if draw == "defaults":
        plans += [("two_low", 30, [lo], False, [lo + 1], True), ("two_high", 30, [hi + 2], False, [hi + 1], True),
                  ("three_short_first", 24, [lo - 1, lo + 4], False, [lo, lo + 4], True),
                  ("three_short_second", 24, [lo + 4, lo - 1], False, [lo + 4, lo], True),
                  ("three_long_first", 24, [hi + 1, hi - 5], False, [hi, hi - 5], True),
                  ("three_long_second", 24, [hi - 5, hi + 1], False, [hi - 5, hi], True),
                  ("three_s1_s2_13", 24, [30, 43], False, [30, 42], True), ("three_s2_s1_13", 24, [43, 30], False, [42, 30], True)]
    else:                                                           # |repeat - spacer| 31 | 30 (-s 20 -S 60)
        plans += [("two_rep_sp_31", 25, [57], False, [56], True), ("three_rep_sp_31", 25, [56, 50], False, [55, 50], True)]
    out = []
    for rep in range(3):
        for sub, n, sa, fa, sb, fb in plans:
            dr = D.dr(n)
            a, b = _plain(D, L, n, sa, found=fa, dr=dr), _plain(D, L, n, sb, found=fb, dr=dr)
            if a and b:
                out.append(Pair("lengths", sub, draw, a, b, dict(n=n, sps=(sa, sb), qc=(a.info["qc"], b.info["qc"]))))
    return kept(out)


@functools.lru_cache(maxsize=None)
def low_complexity_pairs(draw="defaults", L=150, seed=36):
    D = Designer(draw, seed + L)
    out = []
    for n in (23, 24, 32, 33, 40, 47):
        cut = int(n * 0.75)
        for x in LETTERS if 8 + 2 * n + 31 + 1 <= L else ():
            for _ in range(4000):
                d = bytearray([x]) * n
                for q in D.rng.choice(n, n - cut, replace=False):
                    d[int(q)] = D.other(x)[0]
                d = bytes(d)
                ks = [d[i:i + 7] for i in range(n - 6)]
                if len(set(ks)) == len(ks) and d.count(x) == cut:
                    break
            else:
                continue
            qs = [i for i in range(1, n - 1) if d[i] != x]
            q = qs[len(out) % len(qs)]
            d1 = patched(d, q, bytes([x]))
            seq_b, spans = D.array(L, 8, [d, d], [D.spacer(31, 0)])
            seq_a = patched(patched(seq_b, spans[0][0], d1), spans[1][0], d1)
            why = dict(n=n, letter=chr(x), cut_off=cut, count=(d1.count(x), d.count(x)), low=(low_complexity(d1), low_complexity(d)),
                       qc=(qc(seq_a, spans, D.p), qc(seq_b, spans, D.p)))
            out.append(Pair("low_complexity", "n%d_%s" % (n, chr(x)), draw, D.read(seq_a, spans, found=False), D.read(seq_b, spans), why))
    return kept(out)


def _two(D, L, n, at, sp, found=None, lead=None):
    """walk_sets.two_repeats: a two-repeat array with cycling flanks (lead: reached from its last seed offset behind a decoy)"""
    seq, starts = W.two_repeats(D.rng, D.p, L, n, at, sp, (), None, lead)
    if found is None:
        found = int(D.p.lowDRsize) <= n <= int(D.p.highDRsize)
    return D.read(seq, [(s, s + n - 1) for s in starts], found=found, n=n, at=starts[0], lead=lead)


def _lead(D, L, n, sp):
    """a lead decoy (seed 0, distance d) for a repeat of n bases and a spacer of sp: walk_sets.lead_distance's conditions, the
    decoy's seed wholly in front of the repeat"""
    s = E.shape(D.p, L)
    o = n - s.w - (s.w - 2 + s.skips)
    ds = [d for d in range(s.D0, s.D1 + 1) if d + n + sp > s.D1 + s.w and abs(d - (n + sp)) > 24 + s.w and d >= o + s.w + 1]
    if o < 0 or not ds:
        raise AssertionError("no lead")
    return (0, ds[len(ds) // 2])


@functools.lru_cache(maxsize=None)
def extend2(draw="defaults", L=150, seed=37):
    D = Designer(draw, seed + L)
    lo, hi = int(D.p.lowDRsize), int(D.p.highDRsize)
    out = []

    def pair(sub, ra, rb, **why):
        out.append(Pair("extend2", sub, draw, ra, rb, why))

    def sp_of(n):
        return W._sp_low(D.p, n) + 1

    for rep in range(2):
        for off in (0, 4, 7):
            at = 16 - off
            for name, na, nb in (("low", lo - 1, lo), ("high", hi + 1, hi)):
                sp = sp_of(max(na, nb))
                if at + 2 * max(na, nb) + sp < L:
                    pair("%s_off%d" % (name, off), _two(D, L, na, at, sp), _two(D, L, nb, at, sp), n=(na, nb), off=off)
        for name, na, nb in (("low", lo - 1, lo), ("high", hi + 1, hi)):
            sp = W._sp_low(D.p, max(na, nb)) if name == "low" else int(D.p.highSpacerSize)
            rs = []
            for n in (na, nb):
                try:
                    rs.append(_two(D, L, n, None, sp, lead=_lead(D, L, n, sp)))
                except AssertionError:
                    rs = []
                    break
            if rs:
                pair("%s_last" % name, rs[0], rs[1], n=(na, nb))
        sp = sp_of(lo)
        r = [_two(D, L, lo, at, sp) for at in (0, 1, 2)]
        pair("first_at_0|1", r[0], r[1])
        pair("first_at_1|2", r[1], r[2])
        r = [_two(D, L, lo, L - back + 1 - 2 * lo - sp, sp) for back in (1, 2)]
        pair("second_ends_at_L-1|2", r[0], r[1])
        if hi >= 75:
            for side in ("right", "left"):
                for na, nb in ((71, 72), (72, 73)):                     # runs of 63 | 64 and 64 | 65 columns
                    sp = W._sp_low(D.p, nb)
                    rs = []
                    for n in (na, nb):
                        try:
                            if side == "right":
                                rs.append(_two(D, L, n, 8, sp))
                            else:
                                rs.append(_two(D, L, n, None, sp, lead=_lead(D, L, n, sp)))
                        except AssertionError:
                            rs = []
                            break
                    if rs:
                        pair("chunk_%s_%d|%d" % (side, na - 8, nb - 8), rs[0], rs[1], n=(na, nb))
            try:
                pair("chunk_76|75", _two(D, L, 76, 8, W._sp_low(D.p, 76)), _two(D, L, 75, 8, W._sp_low(D.p, 76)), n=(76, 75))
            except AssertionError:
                pass
    return kept(out)


def _votes_read(D, L, n_rep, n, sps, at, rcol=None, lcol=None, dr=None, cut=None):
    """n_rep copies (cut: only that many bases of the last one, the read ends there); rcol / lcol: the base behind / in front of
    copy k (None: they cycle); the columns one further out always cycle"""
    dr = dr or D.dr(n)
    sp = [bytearray(D.spacer(s, k)) for k, s in enumerate(sps)]
    pre, post = bytearray([LETTERS[2], LETTERS[0]]), bytearray([LETTERS[(n_rep - 1) % 4], LETTERS[(n_rep + 1) % 4]])
    for k in range(n_rep):
        if rcol:
            if k < n_rep - 1:
                sp[k][0] = rcol[k]
            else:
                post[0] = rcol[k]
        if lcol:
            if k > 0:
                sp[k - 1][-1] = lcol[k]
            else:
                pre[1] = lcol[k]
    copies = [dr] * n_rep
    if cut:
        copies[-1] = dr[:cut]
        at = L - ((n_rep - 1) * n + sum(sps) + cut)
    if at < 0 or at + (n_rep - 1) * n + sum(sps) + len(copies[-1]) > L:
        return None, None
    seq, spans = D.array(L, at, copies, [bytes(s) for s in sp], pre=bytes(pre), post=bytes(post))
    return seq, spans


def _votes_answer(D, seq, spans, n, el=0, er=0, cut=None):
    """the designed record: every copy el bases to the left and er to the right; a last copy cut to `cut` bases: cut + 1 bases
    in every copy (the column in which extendPreRepeat drops the last copy still passes, the next one does not)"""
    L = len(seq)
    if cut and cut < n:
        spans = [(a, a + cut) for a, b in spans[:-1]] + [(spans[-1][0], L - 1)]
        return D.read(seq, spans, replen=cut + 1)
    spans = [(max(0, a - el), min(L - 1, b + er)) for a, b in spans]
    return D.read(seq, spans, replen=n + el + er)


@functools.lru_cache(maxsize=None)
def votes(draw="defaults", L=251, seed=38):
    D = Designer(draw, seed + L)
    out = []
    n = 26                                                              # (a copy cut by three bases is still lowDR long)
    for n_rep in (3, 4, 5, 7):
        sps = [27 + (k * 2) % 5 for k in range(n_rep - 1)]
        if 16 + n_rep * n + sum(sps) + 2 > L:
            continue
        cut_off = max(2, n_rep - 1)
        for side in ("right", "left"):
            for x in LETTERS:
                rs = []
                dr = D.dr(n)
                for c in (cut_off - 1, cut_off):
                    others = [y for y in LETTERS if y != x]
                    col = [x if k < c else others[(k - c) % 3] for k in range(n_rep)]
                    if side == "left":
                        col = col[::-1]                                 # (the dissenters in front)
                    seq, spans = _votes_read(D, L, n_rep, n, sps, 16, rcol=col if side == "right" else None,
                                             lcol=col if side == "left" else None, dr=dr)
                    ext = int(c >= cut_off)
                    rs.append(_votes_answer(D, seq, spans, n, el=ext if side == "left" else 0, er=ext if side == "right" else 0))
                    rs[-1].info.update(n_rep=n_rep, agree=c, cut_off=cut_off)
                out.append(Pair("votes", "n%d_%s_%s" % (n_rep, side, chr(x)), draw, rs[0], rs[1], dict(n_rep=n_rep, cut_off=cut_off, letter=chr(x))))
        # the last repeat cut by the read's end: whole | one base short | three short
        dr = D.dr(n)
        rs = []
        for cut in (n, n - 1, n - 3):
            seq, spans = _votes_read(D, L, n_rep, n, sps, 0, dr=dr, cut=cut)
            rs.append(seq and _votes_answer(D, seq, spans, n, cut=cut))
        if all(rs):
            out.append(Pair("votes", "n%d_cut_whole|1" % n_rep, draw, rs[0], rs[1], dict(n_rep=n_rep)))
            out.append(Pair("votes", "n%d_cut_1|3" % n_rep, draw, rs[1], rs[2], dict(n_rep=n_rep)))
        # the first repeat at base 0: it has no base in front, the others vote without it: all agree | one dissents
        dr = D.dr(n)
        rs = []
        for agree in (n_rep - 2, n_rep - 1):
            col = [LETTERS[0]] + [LETTERS[1] if k <= agree else LETTERS[2] for k in range(1, n_rep)]
            seq, spans = _votes_read(D, L, n_rep, n, sps, 0, lcol=col, dr=dr)
            rs.append(_votes_answer(D, seq, spans, n, el=int(agree >= cut_off)))
        out.append(Pair("votes", "n%d_first_at_0" % n_rep, draw, rs[0], rs[1], dict(n_rep=n_rep, cut_off=cut_off)))
        # the shortest spacing the second one | the first one
        dr = D.dr(n)
        rs = []
        for order in ((1, 0), (0, 1)):
            s2 = list(sps)
            s2[0], s2[1] = [26, 33][order[0]], [26, 33][order[1]]
            seq, spans = _votes_read(D, L, n_rep, n, s2, 16, dr=dr)
            rs.append(_votes_answer(D, seq, spans, n))
        out.append(Pair("votes", "n%d_shortest_second|first" % n_rep, draw, rs[0], rs[1], dict(n_rep=n_rep)))
    return kept(out)


@functools.lru_cache(maxsize=None)
def chain(draw="defaults", L=251, seed=39):
    D = Designer(draw, seed + L)
    lo, hi = int(D.p.lowSpacerSize), int(D.p.highSpacerSize)
    out = []
    for rep in range(3):
        n = 23 + rep
        for sub, sa, sb in (("cand+25|24", [lo, lo + 25, lo], [lo, lo + 24, lo]), ("cand-25|24", [hi, hi - 25, hi], [hi, hi - 24, hi])):
            dr = D.dr(n)
            rs = []
            for sps in (sa, sb):
                if 8 + 4 * n + sum(sps) + 1 > L:
                    break
                seq, spans = D.array(L, 8, [dr] * 4, [D.spacer(s, k) for k, s in enumerate(sps)])
                # the third copy outside scanRight's window: the first two alone, their spacer measured one base short (lowSp: rejected)
                far = abs(sps[1] - sps[0]) > 24
                rs.append(D.read(seq, spans[:2] if far else spans, found=not (far and sps[0] - 1 < lo), sps=sps))
            if len(rs) == 2:
                out.append(Pair("chain", sub, draw, rs[0], rs[1], dict(n=n, sps=(sa, sb))))
    return kept(out)


def _oriented_dr(D, n, k, lower):
    """a repeat whose first difference from its reverse complement is at base k: lower (the string is its own low-lexi form) or
    higher; k None: a palindrome (n even)"""
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    for _ in range(4000):
        d = bytearray(D.rand(n))
        kk = n // 2 if k is None else k
        for i in range(kk):
            d[i] = comp[d[n - 1 - i]]
        if k is not None:
            if k == n - 1 - k:                                          # the middle base of an odd length: A, C lower, G, T higher
                d[k] = (b"AC" if lower else b"GT")[int(D.rng.integers(0, 2))]
            else:
                c = comp[d[n - 1 - k]]
                pick = [x for x in LETTERS if (x < c if lower else x > c)]
                if not pick:
                    continue
                d[k] = pick[int(D.rng.integers(0, len(pick)))]
        d = bytes(d)
        ks = [d[i:i + 7] for i in range(n - 6)]
        if len(set(ks)) < len(ks) or low_complexity(d):
            continue
        rc = W.revcomp(d)
        first = next((i for i in range(n) if d[i] != rc[i]), None)
        if first == k and (k is None or (d < rc) == lower):
            return d
    return None


@functools.lru_cache(maxsize=None)
def orientation(draw="defaults", L=150, seed=40):
    D = Designer(draw, seed + L)
    hi = int(D.p.highDRsize)
    ns = (23, 31, 32, 33, 47) if hi < 63 else (63, 64, 65, 66, 70, 75)
    pal = (24, 32, 46) if hi < 63 else (64,)
    out = []
    plans = [(n, k, lower) for n in ns for k in sorted({0, 15, 16, 31, 32, (n - 1) // 2} & set(range((n + 1) // 2))) for lower in (True, False)]
    plans += [(n, None, False) for n in pal]
    for i, (n, k, lower) in enumerate(plans):
        d = _oriented_dr(D, n, k, lower)
        sp = W._sp_low(D.p, n) + 1
        at = 0 if i % 3 == 0 else 8 + i % 5                             # every third with the first repeat at base 0
        if d is None or at + 2 * n + sp + 2 > L:
            continue
        seq, spans = D.array(L, at, [d, d], [D.spacer(sp, 0)])
        a = D.read(seq, spans, n=n, first_diff=k, lower=lower, at=at)
        rc = W.revcomp(seq)
        b = D.read(rc, [(L - 1 - y, L - 1 - x) for x, y in reversed(spans)], n=n, first_diff=k, lower=lower)
        why = dict(n=n, first_diff=k, lower=lower, dr=d, at=at, drop="0" if n == 64 else ("<64" if n > 32 else ">=64") if n < 64 else "bytes")
        out.append(Pair("orientation", "n%d_%s_%s%s" % (n, "pal" if k is None else "k%d" % k, "lower" if lower else "higher", "_at0" if at == 0 else ""),
                        draw, a, b, why))
    return kept(out)


@functools.lru_cache(maxsize=None)
def second_round(draw="defaults", L=251, seed=41):
    D = Designer(draw, seed + L)
    out = []
    for i, (n, m) in enumerate([(24, 27), (31, 31), (32, 32), (33, 33), (24, 26), (31, 29)] * 2):
        pr = _sim2_pair(D, "second_round", "n%d_m%d" % (n, m), L, n, m, MODES[i % 3], at=8, behind=(23 + i % 3, 28 + i % 4))
        if pr:
            out.append(pr)
    lo = int(D.p.lowSpacerSize)
    for i in range(4):              # ... rejected by its spacer's length (lowSp - 1 as measured) | accepted (lowSp)
        n = 24 + 3 * i
        dr, dr2, rs = D.dr(n), D.dr(23 + i), []
        for sp in (lo, lo + 1):
            a, keep = D.bg(L), np.zeros(L, bool)
            spans = D.put(a, keep, 8, [dr, dr], [D.spacer(sp, 0)])
            spans2 = D.put(a, keep, 8 + 2 * n + sp + 10, [dr2, dr2], [D.spacer(29 + i, 1)])
            seq = D.finish(a, keep)
            rs.append(D.read(seq, spans2 if sp == lo else spans, qc=qc(seq, spans, D.p)))
        out.append(Pair("second_round", "lengths_n%d" % n, draw, rs[0], rs[1], dict(n=n, sps=(lo, lo + 1), qc=(rs[0].info["qc"], rs[1].info["qc"]))))
    return kept(out)


@functools.lru_cache(maxsize=None)
def field_edges(draw="defaults", L=512, seed=42):
    D = Designer(draw, seed + L)
    out = []
    for back in (1, 2):
        for i, (n, m) in enumerate([(24, 27), (32, 32), (33, 33), (40, 40), (47, 49), (31, 29)]):
            pr = _sim2_pair(D, "field_edges", "ends_at_L-%d_n%d" % (back, n), L, n, m, MODES[(i + back) % 3], end_at=L - back)
            if pr:
                out.append(pr)
    return kept(out)


@functools.lru_cache(maxsize=None)
def pool_reads(n_reads, draw="defaults", L=251, seed=43):
    """exactly n_reads three-repeat arrays, repeat lengths alternating between 32 bases or fewer and more: all found"""
    D = Designer(draw, seed + n_reads)
    out = []
    i = 0
    while len(out) < n_reads:
        i += 1
        n = int(D.rng.integers(23, 33)) if len(out) % 2 == 0 else int(D.rng.integers(33, 48))
        sps = [int(D.rng.integers(27, 36)), 0]
        sps[1] = sps[0] + int(D.rng.integers(-6, 7))
        if sps[1] < 26 or 3 * n + sum(sps) + 2 > L:
            continue
        r = _plain(D, L, n, sps, at=int(D.rng.integers(0, L - (3 * n + sum(sps)) - 1)))
        r.kind, r.sub = "pool", "n%d" % n
        if W.oracle_record(r, D.p) == r.want():
            out.append(r)
        assert i < 6 * n_reads
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the sets
# ---------------------------------------------------------------------------------------------------------------------
PLANS = {       # set: (draw, read length or None for the ragged mix, [(kind function, kwargs)])
    "L150": ("defaults", 150, [(sim2, dict(reps=2)), (words, {}), (transposition, {}), (low_complexity_pairs, {}), (extend2, {}),
                               (orientation, {}), (lengths, {}), (sim3, {}), (votes, {})]),
    "L251": ("defaults", 251, [(sim2, dict(reps=1)), (sim3, {}), (lengths, {}), (votes, {}), (chain, {}), (second_round, {}), (extend2, {}),
                               (transposition, {})]),
    "L400": ("defaults", 400, [(votes, {}), (chain, {}), (second_round, {}), (sim3, {}), (sim2, dict(reps=1)), (lengths, {})]),
    "L512": ("defaults", 512, [(field_edges, {}), (votes, {}), (sim2, dict(reps=1)), (sim3, {}), (second_round, {})]),
    "S20_60": ("S20_60", 251, [(lengths, {}), (sim2, dict(reps=1)), (sim3, {})]),
    "D64S70": ("D64S70", 251, [(words, {}), (sim2, dict(reps=1)), (sim3, {})]),
    "D75": ("D75", 251, [(extend2, {}), (orientation, {}), (sim2, dict(reps=1))]),
}
RAGGED = [(field_edges, 511), (field_edges, 497), (sim2, 100), (sim2, 150), (low_complexity_pairs, 128), (sim3, 200), (votes, 333),
          (orientation, 129), (second_round, 300), (extend2, 177)]
POOLS = {"pool256": 256, "pool257": 257, "pool512": 512}
SETS = tuple(PLANS) + ("ragged",) + tuple(POOLS)


def draw_of(name):
    return PLANS[name][0] if name in PLANS else "defaults"


@functools.lru_cache(maxsize=None)
def pairs_of(name):
    """the kept pairs of a set"""
    if name in POOLS:
        return []
    if name == "ragged":
        return [pr for fn, L in RAGGED for pr in fn("defaults", L)]
    draw, L, kinds = PLANS[name]
    return [pr for fn, kw in kinds for pr in fn(draw, L, **kw)]


@functools.lru_cache(maxsize=None)
def the_set(name):
    """the reads of a set in the order they are run: the kinds mixed (a fixed permutation), twins apart, clean backgrounds to fill
    up to 256 reads; 1 024 at most"""
    if name in POOLS:
        return list(pool_reads(POOLS[name]))
    reads, seen = [], set()
    for pr in pairs_of(name):
        for r in (pr.a, pr.b):
            if id(r) not in seen:                                       # (a read may stand in two pairs: 0 | 1 and 1 | 2)
                seen.add(id(r))
                reads.append(r)
    order = np.random.default_rng(len(reads)).permutation(len(reads))
    reads = [reads[i] for i in order][:1024]
    p = params(draw_of(name))
    lens = sorted({r.L for r in reads})
    k = 0
    while len(reads) < 256:
        L = lens[k % len(lens)]
        bgs = _bg_pool(E.key(p), L)
        r = W.Read(bgs[(k // len(lens) * 5 + 3) % len(bgs)].tobytes(), "background", "background", draw_of(name), False)
        reads.insert((k * 37) % (len(reads) + 1), r)
        k += 1
    return reads
