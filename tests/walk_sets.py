"""Designed reads for pass 1's two long-read kernels (CPU only, seeded, deterministic): the LIGHT WALK (k_long_light,
k_long_light_any: reads of 2 049 .. 12 288 bases and the survivors of 513 .. 2 048 base sets) and the WAVE KERNEL's own forms
of scanRight's chain and extendPreRepeat (k_survivor).  Three parts:

  light_walk(read, params)      a plain restatement of the light walk's control flow -> (verdict, punt_j): 0 "searchCore returns
                                false", 7 "handed over to the full kernel".  Its hint bits are exact ("the w-mer at p stands again
                                D0 .. D1 further on, inside the read"): the kernels' bits are a superset of these, and a seed
                                without the bit finds nothing.  `mutant` names one deliberate slip (MUTANTS: one per edge, mutant_of
                                says which a read is designed for); it exists only so that test_walk_sets_host.py can show that
                                a read's answer hangs on that edge.
  chain(read, params, j, pos)   scanRight's chain from the seed at j and its copy at pos, with the bookkeeping of the wave
                                kernel's match masks (4 096 bases per mask block from a multiple of 64, 64 positions per lane)
  the designed sets, by name    every read carries its kind and the answer WRITTEN DOWN FROM THE DESIGN (found, repeat length,
                                low-lexi flag, start/stops); a read is kept only if orc.search_core gives exactly that answer.

Backgrounds are CLEAN: no position's w-mer stands again D0 .. D1 further on, for any residue class, so a walk meets exactly
the decoys and arrays the design places and nothing else.  A DECOY is one seed's w-mer copied d bases on with different bases
on both sides of the copy: two repeats of w bases, rejected, and the walk goes on at j + d + w - 2 + skips — the designer
picks d to steer the walk into a residue class, onto a given base, or back onto the lattice.

Kinds of the light walk (SETS), under the option draws of DRAWS:
  batch            a decoy moves the walk off the lattice; behind it ONE two-repeat array of lowDR bases whose seeds all lie in
                   one hint word: word cur_base (right behind j and at the word's end), cur_base + 63, + 64, + 127, + 128 (reads
                   of 12 288 bases) and the last word that holds a seed (a read of 12 280 bases: at 12 288 the array's first
                   class seed falls into the word before the last)
  back_to_lattice  two decoys, the second brings the walk back to class 0, the array behind them
  third            -n 3: FOUR repeats with spacers a, a +- 24, a — the third copy is at cand + 24 / cand - 24 of scanRight's
                   first link.  Twins with +- 25 are not found.  ends_at_L: three repeats, spacers 12 apart, the third ends with
                   the read (the link's window is clipped at L; every seed of the repeat sees the third copy, so no read's answer
                   hangs on the clip alone).  (Four, because qcFoundRepeats rejects three repeats whose two spacers differ by
                   more than 12 bases; with a fourth repeat and spacers a, b, a the mean difference is 0.)
  extend           two-repeat arrays that the closed-form extension decides: DR of lowDR reached from its first seed offset (right
                   only), its last (left only, behind a steering decoy) and a middle one (both); DR of highDR; the twins lowDR - 1
                   and highDR + 1; the first repeat at base 0, 1, 2; the second repeat ending at L - 1 and L - 2.  Under
                   -D 75 (k_long_light<true>, D1 = 125): DRs of 72 .. 75 bases from offset 0 (the right run passes the
                   64-base chunk) and from the last offset (the left run does), and the 76-base twin
  any              batch and extend for k_long_light_any (-w 7; -d 20 -D 40; -d 15): hint words counted from word 0 (63, 64, 127,
                   128, the last), and copies of OFF-LATTICE w-mers in front of the real seed in the same hint word (not under
                   -d 15, whose lattice is every base)
  lengths          L = 2 049, 12 225, 12 287, 12 288 with an array in the last 128 bases; L = 12 289 with an array: too long
  dense            513, 1 000, 2 047, 2 048 bases (the survivor list form): extend and third kinds and two exception reads
  turns            8 192 + 64 reads of 2 060 .. 2 200 bases, designed pairs in slots s and s + 8 192

LEFT OUT, by name:
  third / minb     a FOUND third copy at scanRight's lower clamp (last + w + lowSp) is a repeat 34 bases behind the previous
                   one, a spacer of at most 11 bases under DR >= 23: qcFoundRepeats rejects it under every option draw used
                   here.  The reads are in the set with the answer "not found" (the walk hands them over, the full kernel
                   rejects them), but no oracle-found read can depend on the clamp.
  extend / left clamp dependence   with the first repeat at base 0 .. 2 the first seed is on the lattice's first or second point
                   and its left run ends on a mismatch before the clamp: the reads are there, their answer does not hang on it.
  lengths dependence   no slip of its own: at all four lengths the last seed-holding hint word holds fewer than 8 seed positions
                   ((L - 58) mod 64 is 5 .. 7) and an accepted array needs 73 bases from its first seed on, so no found read has all
                   its seeds there.  The reads pin the lengths' own arithmetic (words, hint words, the 12 288 limit) on the GPU.

Kinds of the wave kernel (reads the light walk hands over):
  votes            2, 3, 4, 63, 64, 65, 66 repeats (closed form; lane per repeat up to 64; beyond, column-parallel) whose first
                   flank column agrees in all copies but k = 0, 1, 2 and whose second cycles through ACGT; first repeat at
                   base 0 / 1, last repeat ending at L - 1 / L - 2
  masks            70 and more repeats, spacings searched so that chain links fall on the mask edges, and extra copies of the
                   seed w-mer behind a found repeat, in the window's second lane (labels from chain())
"""
import copy
import functools

import numpy as np

from tests import orc
from tests import edge_reads as E
from tests import long_limit_sets as LS

LL_MAX = 12288                          # LL_HW * 64 * 64: the light walk's longest read
DRAWS = {
    "defaults": {},
    "n3": dict(minNumRepeats=3),
    "D75": dict(highDRsize=75),
    "w7": dict(searchWindowLength=7),
    "d20_D40": dict(lowDRsize=20, highDRsize=40),
    "d15": dict(lowDRsize=15),
}
MUTANTS = {                             # one deliberate slip of light_walk per edge
    "batch_words": "after a class switch the hint words cur_base + 0, 63, 64, 127, 128 and the last seed-holding word are lost",
    "lattice_gone": "the lattice class's words are gone when the walk comes back to class 0",
    "third_window": "scanRight's first link looks 23 bases either side",
    "third_clip": "scanRight's first link's window ends one base before the read does",
    "len_bounds": "lowDR < len < highDR instead of <=",
    "chunk": "a run's second 64-base chunk reads the first one's bases again",
    "right_clamp": "max_right is one base short at the read's end",
    "off_lattice": "k_long_light_any: an off-lattice hint sends the walk to the next hint word",
    "any_words": "k_long_light_any: the hint words 63, 64, 127, 128 and the last seed-holding one are lost",
}


def mutant_of(kind, sub):
    """the slip a read of this kind and sub-case is meant to hang on (None: none)"""
    if kind == "batch":
        return "batch_words"
    if kind == "back_to_lattice":
        return "lattice_gone"
    if kind == "third":
        return {"cand+24": "third_window", "cand-24": "third_window", "ends_at_L": "third_clip"}.get(sub)
    if kind in ("extend", "any"):
        if sub.startswith("batch_"):
            return "any_words"
        if sub == "off_lattice":
            return "off_lattice"
        if sub.startswith("chunk_"):
            return "chunk"
        return "right_clamp" if sub == "second_ends_at_L-1" else "len_bounds"
    return None


def params(draw):
    return orc.Params.default(**DRAWS[draw])


def revcomp(s):
    return LS.revcomp(s)


# ---------------------------------------------------------------------------------------------------------------------
# a) the light walk
# ---------------------------------------------------------------------------------------------------------------------
def _codes(a, w):
    c = E._CODE[a].astype(np.uint32)
    n = len(a) - w + 1
    km = np.zeros(max(n, 0), np.uint32)
    for i in range(w):
        km = (km << 2) | c[i:i + n]
    return km


def hint_bits(read, p):
    """bool per position: the w-mer there stands again D0 .. D1 bases further on, wholly inside the read (ACGT reads)"""
    a = np.frombuffer(read, np.uint8)
    s = E.shape(p, len(a))
    km = _codes(a, s.w)
    bits = np.zeros(len(a), bool)
    for d in range(s.D0, min(s.D1, len(km) - 1) + 1):
        bits[:len(km) - d] |= km[:-d] == km[d:]
    return bits


def light_walk(read, p, mutant=None, trace=None):
    """(verdict, punt_j) of k_long_light (window 8, lattice 8) or k_long_light_any (every other window and lattice) for an ACGT
    read.  trace: a list that receives one dict per candidate (a seed whose copy was found)."""
    L = len(read)
    w, lowDR, highDR, lowSp = int(p.searchWindowLength), int(p.lowDRsize), int(p.highDRsize), int(p.lowSpacerSize)
    highSp, min_rep = int(p.highSpacerSize), int(p.minNumRepeats)
    skips = max(1, lowDR - (2 * w - 1))
    by_class = (w == 8 and skips == 8)
    if (L + 63) >> 6 > LL_MAX // 64:
        return 7, 0
    searchEnd = L - lowDR - lowSp - w - 1
    if searchEnd < 0:
        return 0, 0
    bits = hint_bits(read, p)
    hinted = np.flatnonzero(bits)
    n_hw = (searchEnd >> 6) + 1
    lost_edges = {0, 63, 64, 127, 128}
    assert mutant is None or mutant in MUTANTS
    j, rho, cur_base, switched, frm = 0, 0, 0, False, 0
    gone = False                                    # (mutant lattice_gone)

    def word_lost(pos):
        wd = pos >> 6
        if wd >= n_hw or gone:
            return True
        if mutant == "batch_words" and switched:
            return (wd - cur_base) in lost_edges or wd == ((searchEnd >> 6))
        if mutant == "any_words" and not by_class:
            return wd in lost_edges - {0} or wd == (searchEnd >> 6)
        return False

    def next_hinted(at):
        k = int(np.searchsorted(hinted, at))
        while k < len(hinted):
            q = int(hinted[k])
            if (not by_class or (q & 7) == rho) and not word_lost(q):
                return q
            k += 1
        return None

    while j <= searchEnd:
        q = next_hinted(frm if not by_class else j)
        if q is None or q > searchEnd:
            break
        if not by_class and (q - j) % skips != 0:                # a copy exists there, but it is no seed of this lattice
            frm = ((q | 63) + 1) if mutant == "off_lattice" else q + 1
            continue
        j = q
        begin, end = j + lowDR + lowSp, j + highDR + highSp + w
        if end >= L:
            end = L - 1
        if end < begin:
            end = begin
        if begin > L:
            return 7, j
        pos = read.find(read[j:j + w], begin, end)
        rec = dict(j=j, rho=rho, cur_base=cur_base, batch=(j >> 6) - cur_base, pos=pos)
        if pos < 0:                                             # (cannot happen with exact bits, short of the clamp at L - 1)
            j += skips
            frm = j
            continue
        if trace is not None:
            trace.append(rec)
        # scanRight's first link
        spacing = pos - j
        cand = pos + spacing
        reach = 23 if mutant == "third_window" else 24
        b3, e3 = cand - reach, cand + w + reach
        minb = pos + w + lowSp
        rec.update(cand=cand, minb=minb, third=-1)
        if b3 < minb:
            b3 = minb
        if b3 <= L - 1:
            lim = L - 1 if mutant == "third_clip" else L
            if e3 > lim:
                e3 = lim
            if b3 < e3:
                t = read.find(read[j:j + w], b3, e3)
                if t >= 0:
                    rec.update(third=t, outcome="third")
                    return 7, j
        if 2 < min_rep:
            rec["outcome"] = "two of %d" % min_rep
            j += skips
            frm = j
            continue
        # extendPreRepeat for two repeats, in 64-base chunks
        max_right = spacing - lowSp
        room = L - (pos + w) - (1 if mutant == "right_clamp" else 0)
        if max_right > room:
            max_right = room
        rr = 0
        while rr < max_right:
            nn = min(64, max_right - rr)
            qn = 0
            at = 0 if mutant == "chunk" else rr
            while qn < nn and read[j + w + at + qn] == read[pos + w + at + qn]:
                qn += 1
            rr += qn
            if qn < nn:
                break
        max_left = max(0, spacing - (w + rr))
        if max_left > j:
            max_left = j
        ll = 0
        while ll < max_left:
            nn = min(64, max_left - ll)
            qn = 0
            at = 0 if mutant == "chunk" else ll
            while qn < nn and read[j - at - qn - 1] == read[pos - at - qn - 1]:
                qn += 1
            ll += qn
            if qn < nn:
                break
        replen = w + rr + ll
        rec.update(right=rr, left=ll, replen=replen)
        ok = (lowDR < replen < highDR) if mutant == "len_bounds" else (lowDR <= replen <= highDR)
        if ok:
            rec["outcome"] = "due for qc"
            return 7, j
        rec["outcome"] = "rejected"
        last_end = min(pos + w - 1, L - 1)
        last_end = L - 1 if last_end + rr >= L else last_end + rr
        j = last_end - 1 + skips
        frm = j
        if by_class and (j & 7) != rho:
            rho, cur_base, switched = j & 7, j >> 6, True
            if mutant == "lattice_gone" and rho == 0:
                gone = True
    return 0, 0


# ---------------------------------------------------------------------------------------------------------------------
# b) scanRight's chain with the mask bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def chain(read, p, j, pos):
    """the links of scanRight from the seed at j and its copy at pos -> (found positions, one record per link).  The first link
    is a plain find (base None); from the second on the wave kernel works on match masks: base (first position the masks
    cover), rebuilt, k0 / k1 (lanes of the window's first and last start), bit and lane of the found position, hits (the
    lanes of the window that hold a match), last_p - base, and whether the window was clipped at the read's end."""
    L, w, lowSp = len(read), int(p.searchWindowLength), int(p.lowSpacerSize)
    pat = read[j:j + w]
    found, links = [j, pos], []
    last, spacing, base = pos, pos - j, None
    while True:
        cand = last + spacing
        b, e = cand - 24, cand + w + 24
        if b < last + w + lowSp:
            b = last + w + lowSp
        if b > L - 1:
            break
        clipped = e > L
        if clipped:
            e = L
        if b >= e or e - b < w:
            break
        last_p = e - w
        rec = dict(begin=b, last_p=last_p, clipped=clipped, base=None)
        if len(found) >= 3:
            rebuilt = base is None or b < base or last_p >= base + 4096
            if rebuilt:
                base = b & ~63
            k0, k1 = (b - base) >> 6, (last_p - base) >> 6
            all_hits, at = [], read.find(pat, b, e)
            while at >= 0:
                all_hits.append(at)
                at = read.find(pat, at + 1, e)
            rec.update(base=base, rebuilt=rebuilt, k0=k0, k1=k1, span=last_p - base, hits=sorted({(x - base) >> 6 for x in all_hits}))
        f = read.find(pat, b, e)
        rec["found"] = f
        if f >= 0 and rec["base"] is not None:
            rec.update(bit=(f - base) & 63, lane=(f - base) >> 6, ends_at_L=(f + w == L))
        links.append(rec)
        if f < 0:
            break
        found.append(f)
        spacing, last = f - last, f
        if spacing < lowSp + w:
            break
    return found, links


def chain_plan(starts, L, w=8, lowSp=26, off=0):
    """chain() on a design's repeat starts alone (the seed at offset `off` of every repeat, every link finds the next start):
    the designer's search runs on integers, the read is built for the plan it picks"""
    pts = [s + off for s in starts]
    base, out = None, []
    for k in range(2, len(pts)):
        last, spacing = pts[k - 1], pts[k - 1] - pts[k - 2]
        b, e = max(last + spacing - 24, last + w + lowSp), min(last + spacing + w + 24, L)
        last_p = e - w
        if not (b <= pts[k] <= last_p):
            return None
        if k >= 3:
            rebuilt = base is None or b < base or last_p >= base + 4096
            if rebuilt:
                base = b & ~63
            out.append(dict(base=base, rebuilt=rebuilt, k0=(b - base) >> 6, k1=(last_p - base) >> 6, span=last_p - base,
                            bit=(pts[k] - base) & 63, lane=(pts[k] - base) >> 6, ends_at_L=pts[k] + w == L))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# c) the designed sets
# ---------------------------------------------------------------------------------------------------------------------
class Read:
    """seq; kind / sub (the edge); draw; the designed answer: found, and if so replen, low_lexi, ss (as pass 1 leaves them);
    dep: the design claims that the kind's mutant loses the read"""

    def __init__(self, seq, kind, sub, draw, found, replen=0, low=0, ss=(), dep=True, info=None):
        self.seq, self.kind, self.sub, self.draw, self.found = seq, kind, sub, draw, bool(found)
        self.replen, self.low, self.ss, self.dep, self.info = int(replen), int(low), list(ss), dep and bool(found), info or {}
        self.mutant = mutant_of(kind, sub)                      # the slip this read's answer is meant to hang on

    @property
    def L(self):
        return len(self.seq)

    @property
    def name(self):
        return "%s/%s/%s" % (self.kind, self.sub, self.draw)

    def want(self):
        return (1, self.replen, self.low, self.ss) if self.found else (0,)


def answer(seq, spans, replen=None):
    """the record of an array whose repeats are spans [(start, stop)] in seq: (replen, low_lexi, ss) as pass 1 leaves them.
    The repeat that names the DR is the second (of two repeats: the first, if it is the longer one and does not start the
    read — ReadHolder::DRLowLexi); ss as placed when that string is its own low-lexi form, mirrored when its reverse
    complement is the smaller.  replen: RH_RepeatLength where a span is clipped at the read's end"""
    pick = 1
    if len(spans) == 2 and spans[0][0] != 0 and spans[0][1] - spans[0][0] > spans[1][1] - spans[1][0]:
        pick = 0
    a, b = spans[pick]
    dr = seq[a:b + 1]
    ss = [x for sp in spans for x in sp]
    if replen is None:
        replen = max(y - x + 1 for x, y in spans)
    if dr < revcomp(dr):
        return replen, 1, ss
    return replen, 0, [len(seq) - 1 - x for x in reversed(ss)]


def oracle_record(r, p=None):
    """orc.search_core's answer in the form of Read.want()"""
    p = p or params(r.draw)
    f, ss, rl = orc.search_core(r.seq, p)
    if f != 1:
        return (0,)
    return (1,) + answer(r.seq, [(ss[i], ss[i + 1]) for i in range(0, len(ss), 2)], rl)


def kept(reads):
    """the reads whose designed answer is the oracle's"""
    return [r for r in reads if oracle_record(r) == r.want()]


def clean(a, p, rng, keep=None):
    """in place: no w-mer of the rows of a (n, L) stands again D0 .. D1 further on.  Positions under `keep` (bool (n, L)) are
    not changed, and a pair whose two w-mers lie wholly under it is the design's own and stays."""
    n, L = a.shape
    s = E.shape(p, L)
    m = L - s.w + 1
    if keep is not None:                                        # w-mers wholly under keep
        cs = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(keep, axis=1)], axis=1)
        whole = (cs[:, s.w:] - cs[:, :m]) == s.w
    act = np.arange(n)                                          # the rows that still held a pair in the last round
    for _ in range(500):
        c = E._CODE[a[act]].astype(np.uint32)
        km = np.zeros((len(act), m), np.uint32)
        for i in range(s.w):
            km = (km << 2) | c[:, i:i + m]
        rs, qs = [], []
        for d in range(s.D0, min(s.D1, m - 1) + 1):
            r, q = np.nonzero(km[:, :m - d] == km[:, d:])
            r = act[r]
            if len(r) and keep is not None:
                mine = whole[r, q] & whole[r, q + d]
                r, q = r[~mine], q[~mine]
            if len(r):
                side = rng.integers(0, 2, size=len(r))           # a base of the w-mer or of its copy
                rs.append(r)
                qs.append(q + side * d + rng.integers(0, s.w, size=len(r)))
        if not rs:
            return a
        r, q = np.concatenate(rs), np.concatenate(qs)
        act = np.unique(r)
        if keep is not None:
            ok = ~keep[r, q]
            r, q = r[ok], q[ok]
        a[r, q] = E.LETTERS[(E._CODE[a[r, q]] + rng.integers(1, 4, size=len(r))) & 3]
    raise AssertionError("clean: no fixed point")


def background(rng, p, L, n=1):
    return clean(E.LETTERS[rng.integers(0, 4, size=(n, L))], p, rng)


def _other(rng, *not_these):
    """a letter different from the given bytes"""
    return int(rng.choice([c for c in E.LETTERS if c not in not_these]))


def decoy(rng, a, jd, d, w):
    """the w-mer at jd again at jd + d, the bases on both sides of the copy different from the original's"""
    E._plant(a, jd, jd + d, w)
    if jd + d + w < len(a):
        a[jd + d + w] = _other(rng, a[jd + w])
    if jd > 0:
        a[jd + d - 1] = _other(rng, a[jd - 1])


def steer(p, L, jd, target):
    """the decoy distance that sends the walk from the seed jd onto base `target`"""
    s = E.shape(p, L)
    d = target - (s.w - 2 + s.skips) - jd
    assert s.D0 <= d <= s.D1, (jd, target, d)
    return d


def random_dr(rng, n, w, flipped=None):
    """a repeat of n bases: no (w - 1)-mer twice, not low-complexity, low-lexi form as asked (None: either)"""
    while True:
        d = E._rand(rng, n).tobytes()
        ks = [d[i:i + w - 1] for i in range(n - w + 2)]
        if len(set(ks)) < len(ks) or orc.lib().orc_is_low_complexity(d, n) or d == revcomp(d):
            continue
        if flipped is None or (revcomp(d) < d) == flipped:
            return d


def lay(rng, a, dr, starts, w, left=None, right=None):
    """copies of dr at starts in a (in place).  left / right: the base next to copy k (None: they cycle through ACGT, so that no
    column passes a vote); the column behind that one always cycles.  Spacers: no (w - 1)-mer of the repeat, flanks kept.
    Returns the mask of the bases it placed."""
    d = np.frombuffer(dr, np.uint8)
    n, L = len(d), len(a)
    fixed = np.zeros(L, bool)
    for st in starts:
        a[st:st + n] = d
        fixed[st:st + n] = True
    for k, st in enumerate(starts):
        for off, col in ((-1, left), (n, right)):
            for depth in (0, 1):                                 # the column next to the repeat, and the one behind it
                q = st + off + (depth if off > 0 else -depth)
                if 0 <= q < L and not fixed[q]:
                    if depth == 0 and col is not None:
                        a[q] = col[k]
                    else:
                        a[q] = E.LETTERS[(k + depth + (1 if off > 0 else 0)) % 4]
                    fixed[q] = True
    kmers = {dr[i:i + w - 1] for i in range(n - w + 2)}
    for k in range(len(starts) - 1):
        lo, hi = starts[k] + n, starts[k + 1]
        for _ in range(200):
            bad = [i for i in range(lo - w + 2, hi) if a[i:i + w - 1].tobytes() in kmers and not fixed[i:i + w - 1].all()]
            if not bad:
                break
            for i in bad:
                free = [q for q in range(i, i + w - 1) if not fixed[q]]
                q = int(rng.choice(free))
                a[q] = _other(rng, a[q])
    return fixed


def lead_distance(p, L, n_dr, sp):
    """a distance for a LEAD decoy: the copy of its seed is a w-mer of the first repeat; neither is the second repeat's copy in
    the seed's window, nor where scanRight's first link looks"""
    s = E.shape(p, L)
    ds = [d for d in range(s.D0, s.D1 + 1) if d + n_dr + sp > s.D1 + s.w and abs(d - (n_dr + sp)) > 24 + s.w]
    assert ds, (n_dr, sp)
    return ds[len(ds) // 2]


def two_repeats(rng, p, L, n_dr, at, sp, decoys=(), flipped=None, lead=None):
    """a clean read of L bases with the decoys [(jd, d)] and a two-repeat array (DR of n_dr bases at `at`, spacer sp).
    lead = (jd, d): `at` is chosen so that the decoy seed at jd is a w-mer of the first repeat, d bases before its place
    there, the one after whose rejection the walk goes on at the repeat's LAST seed offset (n_dr - w); the bases next to the
    w-mer at jd differ from the repeat's."""
    s = E.shape(p, L)
    a = background(rng, p, L)[0]
    dr = random_dr(rng, n_dr, s.w, flipped)
    if lead:
        jd, d = lead
        o = n_dr - s.w - (s.w - 2 + s.skips)
        assert o >= 0
        at = jd + d - o
    starts = [at, at + n_dr + sp]
    assert starts[1] + n_dr <= L, (L, at, n_dr, sp)
    keep = lay(rng, a, dr, starts, s.w)
    if lead:
        a[jd:jd + s.w] = np.frombuffer(dr[o:o + s.w], np.uint8)
        a[jd + s.w] = _other(rng, dr[o + s.w])
        if jd > 0:
            a[jd - 1] = _other(rng, dr[o - 1] if o else a[at - 1])
        keep[max(0, jd - 1):jd + s.w + 1] = True
    for jd_, d_ in decoys:
        decoy(rng, a, jd_, d_, s.w)
        keep[jd_:jd_ + s.w] = True
        keep[max(0, jd_ + d_ - 1):jd_ + d_ + s.w + 1] = True
    keep[max(0, starts[0] - 2):starts[1] + n_dr + 2] = True
    clean(a.reshape(1, -1), p, rng, keep.reshape(1, -1))
    return a.tobytes(), starts


def _two(kind, sub, draw, rng, L, n_dr, at, sp, decoys=(), dep=True, flipped=None, info=None, lead=None):
    p = params(draw)
    seq, starts = two_repeats(rng, p, L, n_dr, at, sp, decoys, flipped, lead)
    found = int(p.lowDRsize) <= n_dr <= int(p.highDRsize)
    rl, low, ss = answer(seq, [(st, st + n_dr - 1) for st in starts])
    return Read(seq, kind, sub, draw, found, rl, low, ss, dep, dict(info or {}, at=starts[0], n_dr=n_dr, decoys=list(decoys), lead=lead))


def _sp_low(p, n_dr):
    return max(int(p.lowSpacerSize) + 1, n_dr - 30 + 1)


def _sp(rng, p, n_dr):
    """a spacer two repeats of n_dr bases are accepted with (qcFoundRepeats measures it one base short)"""
    lo = _sp_low(p, n_dr)
    return int(rng.integers(lo, min(int(p.highSpacerSize) + 1, lo + 10) + 1))


@functools.lru_cache(maxsize=None)
def batch_set(draw="defaults", seed=1, reps=2):
    p = params(draw)
    rng = np.random.default_rng([seed, 11] + list(E.key(p)))
    s = E.shape(p, LL_MAX)
    n_dr, span = int(p.lowDRsize), int(p.lowDRsize) - s.w                   # the seeds of the repeat: at .. at + span
    out = []
    for rep in range(reps):
        for sub in ("w0_behind_j", "w0_end", "w63", "w64", "w127", "w128", "last"):
            L = LL_MAX
            if s.skips == 8 and s.w == 8:
                rho = 1 + (len(out) % 7)
                jd = 8 * int(rng.integers(0, 4))
                d = [x for x in range(s.D0 + 8, s.D0 + 16) if (jd + x + 14) & 7 == rho and (jd + x + 14) & 63 <= 40][0]
                j0 = jd + d + 14
                decoys, cb = [(jd, d)], j0 >> 6
            else:
                decoys, cb, j0 = [], 0, 0
            sp = _sp(rng, p, n_dr)
            if sub == "w0_behind_j":
                if not decoys:
                    continue
                at = j0
            elif sub == "w0_end":
                if not decoys:
                    continue
                at = (cb << 6) + 63 - span
            elif sub == "last":
                # a length whose last seed-holding word holds every seed of an array that ends with the read's last base but one
                L = [x for x in range(LL_MAX, LL_MAX - 64, -1) if (x - 1 - 2 * n_dr - sp) >> 6 == (x - 1 - 2 * n_dr - sp + span) >> 6 ==
                     (E.shape(p, x).searchEnd >> 6)][0]
                at = L - 1 - 2 * n_dr - sp
            else:
                k = int(sub[1:])
                at = ((cb + k) << 6) + int(rng.integers(0, 64 - span))
            out.append(_two("batch" if decoys else "any", ("batch_" if not decoys else "") + sub, draw, rng, L, n_dr, at, sp, decoys,
                            info=dict(word=at >> 6, cur_base=cb)))
    return kept(out)


@functools.lru_cache(maxsize=None)
def back_to_lattice_set(draw="defaults", seed=2, n=10):
    p = params(draw)
    rng = np.random.default_rng([seed, 12] + list(E.key(p)))
    s = E.shape(p, 4000)
    out = []
    for i in range(n):
        L = int(rng.integers(2100, LL_MAX + 1))
        jd = 8 * int(rng.integers(0, 30))
        rho = 1 + i % 7
        d1 = [x for x in range(s.D0, s.D1) if (jd + x + 14) & 7 == rho][int(rng.integers(0, 5))]
        j1 = jd + d1 + 14 + 8 * int(rng.integers(0, 20))                 # a seed of class rho further on
        d2 = [x for x in range(s.D0, s.D1) if (j1 + x + 14) & 7 == 0][int(rng.integers(0, 5))]
        j2 = j1 + d2 + 14
        n_dr = int(p.lowDRsize)
        at = j2 + int(rng.integers(0, min(600, L - j2 - 120)))
        out.append(_two("back_to_lattice", "class%d" % rho, draw, rng, L, n_dr, at, _sp(rng, p, n_dr), [(jd, d1), (j1, d2)], flipped=bool(i & 1)))
    return kept(out)


def _four(kind, sub, draw, rng, L, n_dr, at, sps, found, dep=True, end_at=None):
    p = params(draw)
    s = E.shape(p, L)
    a = background(rng, p, L)[0]
    dr = random_dr(rng, n_dr, s.w)
    if end_at is not None:
        at = end_at - (len(sps) + 1) * n_dr - sum(sps)
    starts = [at]
    for sp in sps:
        starts.append(starts[-1] + n_dr + sp)
    keep = lay(rng, a, dr, starts, s.w)
    keep[max(0, starts[0] - 2):min(L, starts[-1] + n_dr + 2)] = True
    clean(a.reshape(1, -1), p, rng, keep.reshape(1, -1))
    seq = a.tobytes()
    rl, low, ss = answer(seq, [(st, st + n_dr - 1) for st in starts])
    return Read(seq, kind, sub, draw, found, rl, low, ss, dep, dict(at=at, starts=starts))


@functools.lru_cache(maxsize=None)
def third_set(draw="n3", seed=3, lengths=(2100, 5000, 9000, LL_MAX), reps=3):
    p = params(draw)
    rng = np.random.default_rng([seed, 13] + list(E.key(p)))
    out = []
    lo, hi = int(p.lowSpacerSize), int(p.highSpacerSize)
    for rep in range(reps):
        for L in lengths:
            n_dr = int(rng.integers(int(p.lowDRsize) + 1, int(p.lowDRsize) + 8))
            at = int(rng.integers(0, L - 400))
            out.append(_four("third", "cand+24", draw, rng, L, n_dr, at, [lo, lo + 24, lo], True))
            out.append(_four("third", "cand-24", draw, rng, L, n_dr, at, [hi, hi - 24, hi], True))
            out.append(_four("third", "cand+25", draw, rng, L, n_dr, at, [lo, lo + 25, lo], False))
            out.append(_four("third", "cand-25", draw, rng, L, n_dr, at, [hi, hi - 25, hi], False))
            # three repeats, the third ends with the read: the first link's window is clipped at L (spacers 12 apart: accepted)
            out.append(_four("third", "ends_at_L", draw, rng, L, n_dr, None, [lo + 12, lo], True, dep=False, end_at=L))
            # a copy of the seed at scanRight's lower clamp: a stub of a third repeat 34 bases behind the second (handed over, rejected)
            out.append(_four("third", "minb", draw, rng, L, n_dr, at, [lo, 8 + lo - n_dr], False))
    return kept(out)


@functools.lru_cache(maxsize=None)
def extend_set(draw="defaults", seed=4, lengths=(2100, 6000, LL_MAX), kind="extend"):
    p = params(draw)
    rng = np.random.default_rng([seed, 14] + list(E.key(p)))
    lowDR, highDR = int(p.lowDRsize), int(p.highDRsize)
    out = []
    for L in lengths:
        s = E.shape(p, L)
        lat = lambda x: -(-x // s.skips) * s.skips                  # the lattice point at or behind x

        def add(sub, n_dr, at, decoys=(), dep=True, sp=None, lead=False):
            sp = sp or (_sp_low(p, n_dr) if lead else _sp(rng, p, n_dr))
            ld = (mid, lead_distance(p, L, n_dr, sp)) if lead else None
            out.append(_two(kind, sub, draw, rng, L, n_dr, at, sp, decoys, dep, flipped=bool(len(out) & 1), lead=ld))

        mid = lat(int(rng.integers(L // 4, L // 2)))
        span = lowDR - s.w
        add("low_right_only", lowDR, mid)                           # the seed at DR offset 0
        if s.skips > 1:
            add("low_both", lowDR, mid - min(span - 1, s.skips - 1))
        add("low_left_only", lowDR, None, lead=True)                # the seed at the last offset, behind a lead decoy
        add("high", highDR, mid)
        add("low-1", lowDR - 1, mid)
        add("high+1", highDR + 1, mid)
        for at in (0, 1, 2):
            add("first_at_%d" % at, lowDR, at, dep=False)
        for back in (1, 2):
            sp = _sp(rng, p, lowDR)
            add("second_ends_at_L-%d" % back, lowDR, L - back + 1 - 2 * lowDR - sp, sp=sp, dep=back == 1)
        if highDR >= 72:
            for n_dr in (72, 73, 74, 75):
                add("chunk_right_%d" % n_dr, n_dr, mid)
                add("chunk_left_%d" % n_dr, n_dr, None, lead=True)
            add("chunk_76", 76, mid)
    return kept(out)


@functools.lru_cache(maxsize=None)
def any_set(draw, seed=5):
    """k_long_light_any: the batch words, the extension's edges, and off-lattice copies in front of the real seed"""
    p = params(draw)
    rng = np.random.default_rng([seed, 15] + list(E.key(p)))
    s = E.shape(p, LL_MAX)
    assert not (s.w == 8 and s.skips == 8)
    out = list(batch_set(draw)) + list(extend_set(draw, lengths=(2100, LL_MAX), kind="any"))
    if s.skips > 1:
        n_dr = int(p.lowDRsize)
        for i in range(16):
            L = LL_MAX if i & 1 else int(rng.integers(2100, 9000))
            wd = int(rng.integers(2, (L - 300) >> 6))
            at = (wd << 6) + int(rng.integers(12, 64 - (n_dr - s.w)))
            sp = _sp_low(p, n_dr)
            end = at + 2 * n_dr + sp
            offs = [q for q in range(at - 10, at - 1) if q % s.skips != 0 and (q >> 6) == wd]
            decs = [(q, end + 3 + 11 * k - q) for k, q in enumerate(offs[-2:])]
            decs = [(q, d) for q, d in decs if s.D0 <= d <= s.D1]
            if not decs:
                continue
            r = _two("any", "off_lattice", draw, rng, L, n_dr, at, sp, decs, flipped=bool(i & 2))
            r.info["off"] = [q for q, _ in decs]
            out.append(r)
    return kept(out)


@functools.lru_cache(maxsize=None)
def lengths_set(draw="defaults", seed=6):
    p = params(draw)
    rng = np.random.default_rng([seed, 16] + list(E.key(p)))
    out = []
    n_dr = int(p.lowDRsize)
    for L in (2049, 12225, 12287, 12288, 12289):
        sp = _sp(rng, p, n_dr)
        # the array ends with the read's last base but one; all of it in the last 128 bases
        at = L - 1 - 2 * n_dr - sp
        assert at >= L - 128
        out.append(_two("lengths", "L%d" % L, draw, rng, L, n_dr, at, sp, dep=False))
    return kept(out)


def _exception_read(rng, p, L):
    """a real array with an N in its spacer"""
    n_dr = int(p.lowDRsize) + 4
    r = _four("dense", "exception_N", "defaults", rng, L, n_dr, int(rng.integers(0, L - 300)), [30, 32, 31], True, dep=False)
    st = r.info["starts"]
    b = bytearray(r.seq)
    b[st[1] + n_dr + 12] = ord("N")
    r.seq = bytes(b)
    return r


@functools.lru_cache(maxsize=None)
def dense_set(draw="defaults", seed=7):
    """reads of 513 .. 2 048 bases: the survivor list form.  ACGT backgrounds between the designed reads."""
    p = params(draw)
    rng = np.random.default_rng([seed, 17] + list(E.key(p)))
    lens = (513, 1000, 2047, 2048)
    if int(p.minNumRepeats) >= 3:
        out = list(third_set(draw, seed=seed, lengths=lens, reps=1))
    else:
        out = list(extend_set(draw, seed=seed, lengths=lens, kind="extend" if draw == "defaults" else "any"))
    out = [copy.copy(r) for r in out]
    for r in out:
        r.kind = "dense"                                        # (r.mutant stays: the kind the read was designed as)
    if draw == "defaults":
        for L in (1000, 2048):
            out.insert(len(out) // 2, _exception_read(rng, p, L))
    out = kept(out)
    bgs = [Read(background(rng, p, L)[0].tobytes(), "dense", "background", draw, False) for L in lens for _ in range(4)]
    mixed = []
    for i, r in enumerate(out):
        mixed.append(r)
        if i % 3 == 0:
            mixed.append(bgs[(i // 3) % len(bgs)])
    return mixed


TURN_SLOTS = 8192                       # the light walk's grid: 256 x 32 blocks


@functools.lru_cache(maxsize=None)
def turns_set(draw="defaults", seed=8, extra=64):
    """8 192 + 64 reads: the blocks 0 .. 63 take a second read.  Slots s and s + 8 192 (s < 64) hold designed pairs — a 12 288-base
    batch read and a short extend read, in both orders; the rest is clean background of 2 060 .. 2 200 bases."""
    p = params(draw)
    rng = np.random.default_rng([seed, 18] + list(E.key(p)))
    n = TURN_SLOTS + extra
    lens = rng.integers(2060, 2201, size=n)
    bg = background(rng, p, 2200, n)
    reads = [Read(bg[i, :lens[i]].tobytes(), "turns", "background", draw, False) for i in range(n)]
    big = list(batch_set(draw))
    small = [r for r in extend_set(draw) if r.L < 3000]
    for s in range(extra):
        a, b = big[s % len(big)], small[s % len(small)]
        if (s // 2) & 1:
            a, b = b, a
        if s % 2 == 0:                                          # (every other pair: a neighbour block's second read stays background)
            reads[s], reads[s + TURN_SLOTS] = a, b
    return reads


def turns_designed(reads):
    return [i for i, r in enumerate(reads) if r.sub != "background"]


# ---- the wave kernel's forms ----
VOTE_COUNTS = (2, 3, 4, 63, 64, 65, 66)


def _vote_passes(col, n_rep):
    """extendPreRepeat's vote on one column: the voters' bases -> does a base reach max(2, repeats - 1)"""
    return max(col.count(c) for c in set(col)) >= max(2, n_rep - 1) if col else False


def _votes_read(rng, p, L, n_rep, k, place, draw):
    dr = LS.DR_A
    n = len(dr)
    a = background(rng, p, L)[0]
    gaps = [int(rng.integers(30, 41)) for _ in range(n_rep - 1)]
    span = n_rep * n + sum(gaps)
    # the first repeat on a lattice point (one base behind it, the lattice seed would hold the agreeing flank column, and
    # scanRight's chain would not link the dissenters): the read's length gives way
    if place.startswith("ends_at_L-"):
        back = int(place[-1]) - 1
        L -= (L - back - span) % 8
    first = {"first_at_0": 0, "first_at_1": 1, "ends_at_L-1": L - span, "ends_at_L-2": L - 1 - span}.get(place)
    if first is None:
        first = 8 * int(rng.integers(8, (L - span - 70) // 8))
    a = a[:L]
    starts = [first]
    for g in gaps:
        starts.append(starts[-1] + n + g)
    # the dissenters of the first column: the last repeat, then the first, then the middle one — all with the same other base
    who = [n_rep - 1, 0, n_rep // 2][:k]
    if n_rep == 2 and k == 2:
        who = [1]
    left = [ord("G") if i in who else ord("A") for i in range(n_rep)]
    right = [ord("A") if i in who else ord("G") for i in range(n_rep)]
    if n_rep == 2 and k == 2:
        left, right = [ord("C"), ord("G")], [ord("T"), ord("A")]
    keep = lay(rng, a, dr, starts, 8, left, right)
    keep[max(0, starts[0] - 2):min(L, starts[-1] + n + 2)] = True
    clean(a.reshape(1, -1), p, rng, keep.reshape(1, -1))
    seq = a.tobytes()
    # the answer, from the design: a column's voters are the copies whose base of that column is on the read
    rvote = [right[i] for i, st in enumerate(starts) if st + n < L]
    lvote = [left[i] for i, st in enumerate(starts) if st - 1 >= 0]
    # (extendPreRepeat drops the last copy for a column at or past the read's end, and the first for one before its start)
    er = 1 if _vote_passes(rvote, n_rep) else 0
    el = 1 if _vote_passes(lvote, n_rep) else 0
    spans = [(max(0, st - el), min(L - 1, st + n - 1 + er)) for st in starts]
    rl, low, ss = answer(seq, spans, n + er + el)
    return Read(seq, "votes", "n%d_k%d_%s" % (n_rep, k, place), draw, True, rl, low, ss, False,
                dict(starts=starts, n_rep=n_rep, k=k, ext=(el, er), place=place))


@functools.lru_cache(maxsize=None)
def votes_set(draw="defaults", seed=9):
    p = params(draw)
    rng = np.random.default_rng([seed, 19] + list(E.key(p)))
    out = []
    for n_rep in VOTE_COUNTS:
        L = 2100 if n_rep <= 4 else 6000
        for k in (0, 1, 2):
            out.append(_votes_read(rng, p, L, n_rep, k, "middle", draw))
        for place in ("first_at_0", "first_at_1", "ends_at_L-1", "ends_at_L-2"):
            out.append(_votes_read(rng, p, L, n_rep, 0, place, draw))
            if place != "first_at_1":                           # (there the seed at base 0 holds the flank column: no dissenter)
                out.append(_votes_read(rng, p, L, n_rep, 1, place, draw))
    return kept(out)


MASK_LABELS = ("bit63", "bit0_next_lane", "second_lane_only", "both_lanes", "span4095_kept", "span4096_rebuilt", "ends_at_L")


def _plan_labels(plan):
    lab, base = set(), None
    for r in plan:
        if r["bit"] == 63:
            lab.add("bit63")
        if r["k1"] > r["k0"] and r["lane"] == r["k1"]:
            lab.add("second_lane_only")
            if r["bit"] == 0:
                lab.add("bit0_next_lane")
        if not r["rebuilt"] and r["span"] == 4095:
            lab.add("span4095_kept")
        if r["rebuilt"] and base is not None and r["base"] + r["span"] - base == 4096:
            lab.add("span4096_rebuilt")
        if r["ends_at_L"]:
            lab.add("ends_at_L")
        if len(r.get("hits", ())) == 2 and r["lane"] == r["k0"] == r["hits"][0]:
            lab.add("both_lanes")                                # (chain()'s records only: a plan holds no text)
        base = r["base"]
    return lab


def _both_lane_spots(starts, plan, L, w, n):
    """where an extra copy of the seed w-mer (seed offset 0) makes a link's window hold a match in two lanes: two bases behind
    the found repeat's second flank column, in the next lane, still a start of this link's window — and in front of the next
    link's, which begins last + w + lowSp on at the earliest"""
    out = []
    for i, r in enumerate(plan):
        k = i + 3
        f, x = starts[k], starts[k] + n + 2
        cand = 2 * starts[k - 1] - starts[k - 2]
        last_p = min(cand + w + 24, L) - w
        if r["lane"] == r["k0"] and (x - r["base"]) >> 6 == r["lane"] + 1 and x <= last_p and (k + 1 == len(starts) or starts[k + 1] - f >= 57):
            out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def masks_set(draw="defaults", seed=10, per_label=8):
    """arrays of 70 and more copies of DR_A in reads of up to 12 288 bases.  The spacings (56 .. 80 bases from start to start, a
    step of at most 24 between neighbours) are searched on integers (chain_plan) until every label of MASK_LABELS has
    per_label reads; the reads are then built and labelled again from chain() on their text.  ends_at_L: the seed is the
    repeat's LAST w-mer (a decoy steers the walk onto it), so the last link's window start is L - w, the last bit n_ok keeps.

    both_lanes: an extra copy of the seed w-mer in the spacer BEHIND a found repeat, in the next lane of the same window (the
    spacing shrinks by 8 bases or more at that link, so the window still reaches it): the leftmost wins, the record holds the
    repeat and not the extra copy, and chain() records hits in two lanes.  (In the lane BEFORE the real one it cannot be: the window
    begins last + w + lowSp on, a "repeat" with a spacer of 4 bases ends the chain and fails qcFoundRepeats.)"""
    p = params(draw)
    rng = np.random.default_rng([seed, 20] + list(E.key(p)))
    n, w = 30, 8
    need = {lab: per_label for lab in MASK_LABELS}
    plans = []
    for _ in range(200000):
        if not any(v > 0 for v in need.values()):
            break
        tail = bool(rng.integers(0, 2)) if need["ends_at_L"] > 0 else False
        n_rep = int(rng.integers(70, 150))
        gaps = [int(rng.integers(62, 75))]
        for _k in range(n_rep - 2):
            gaps.append(int(np.clip(gaps[-1] + rng.integers(-10, 11), 57, 79)))
        span = sum(gaps) + n
        L = int(rng.integers(max(span + 300, 6000), LL_MAX + 1)) if span + 300 < LL_MAX else 0
        if not L:
            continue
        if tail:
            first = L - span
            off = n - w
            if first < 200:
                continue
        else:
            first, off = 8 * int(rng.integers(4, (L - span - 40) // 8)), 0
        starts = list(np.cumsum([first] + gaps))
        plan = chain_plan(starts, L, w, int(p.lowSpacerSize), off)
        if plan is None:
            continue
        lab = _plan_labels(plan)
        starts = [int(x) for x in starts]
        extras = _both_lane_spots(starts, plan, L, w, n)[:2] if off == 0 and need["both_lanes"] > 0 else []
        if extras:
            lab.add("both_lanes")
        if any(need[x] > 0 for x in lab):
            plans.append((L, starts, off, tail, extras))
            for x in lab:
                need[x] -= 1
    out = []
    for L, starts, off, tail, extras in plans:
        a = background(rng, p, L)[0]
        keep = lay(rng, a, LS.DR_A, starts, w)
        for x in extras:
            a[x:x + w] = np.frombuffer(LS.DR_A[:w], np.uint8)
        keep[max(0, starts[0] - 2):min(L, starts[-1] + n + 2)] = True
        decs = []
        if tail:
            target = starts[0] + off
            jd = 8 * ((target - 100) // 8)
            decs = [(jd, steer(p, L, jd, target))]
            decoy(rng, a, jd, decs[0][1], w)
            keep[jd:jd + w] = True
            keep[jd + decs[0][1] - 1:jd + decs[0][1] + w + 1] = True
        clean(a.reshape(1, -1), p, rng, keep.reshape(1, -1))
        seq = a.tobytes()
        rl, low, ss = answer(seq, [(st, st + n - 1) for st in starts])
        _, links = chain(seq, p, starts[0] + off, starts[1] + off)
        lab = _plan_labels([r for r in links if r["base"] is not None and r["found"] >= 0])
        out.append(Read(seq, "masks", "+".join(sorted(lab)) or "none", draw, True, rl, low, ss, False,
                        dict(starts=starts, off=off, labels=lab, decoys=decs, extras=extras)))
    return kept(out)


LIGHT_SETS = {
    ("batch", "defaults"): lambda: batch_set("defaults"),
    ("back_to_lattice", "defaults"): lambda: back_to_lattice_set("defaults"),
    ("third", "n3"): lambda: third_set("n3"),
    ("extend", "defaults"): lambda: extend_set("defaults"),
    ("extend", "D75"): lambda: extend_set("D75"),
    ("any", "w7"): lambda: any_set("w7"),
    ("any", "d20_D40"): lambda: any_set("d20_D40"),
    ("any", "d15"): lambda: any_set("d15"),
    ("lengths", "defaults"): lambda: lengths_set("defaults"),
    ("dense", "defaults"): lambda: dense_set("defaults"),
    ("dense", "n3"): lambda: dense_set("n3"),
    ("dense", "w7"): lambda: dense_set("w7"),
}
WAVE_SETS = {
    ("votes", "defaults"): lambda: votes_set("defaults"),
    ("masks", "defaults"): lambda: masks_set("defaults"),
}


def get(kind, draw):
    return list((LIGHT_SETS.get((kind, draw)) or WAVE_SETS[(kind, draw)])())


@functools.lru_cache(maxsize=None)
def gpu_set(kind, draw, at_least=96):
    """the set as test_gpu_long_walk.py runs it: the designed reads with clean backgrounds of their lengths between them, 96
    reads at least (more than 64: an explicit CRASS_HINT_PARTS slices the set)"""
    reads = get(kind, draw)
    p = params(draw)
    rng = np.random.default_rng([99, len(reads)] + list(E.key(p)))
    lens = sorted({r.L for r in reads})
    n_bg = max(at_least - len(reads), len(reads) // 4)
    bgs = [Read(background(rng, p, lens[i % len(lens)])[0].tobytes(), kind, "background", draw, False) for i in range(n_bg)]
    out = list(reads)
    for i, b in enumerate(bgs):                                  # spread evenly, the set's first and last read designed ones
        out.insert(1 + (i * (len(out) - 1)) // n_bg, b)
    return out
