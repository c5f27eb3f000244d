"""The DR merge (WorkHorse::createNonRedundantSet = clusterDRReads + removeRedundantRepeats, WorkHorse.cpp:612-709, 1404-1637) on
designed token sets: the plain reference, the named sets that reach every branch of the device merge (dmerge.hip) and of the
pass-2 tables it builds, and designed pass-2 reads over the reference's patterns.  No GPU, no product code: bytes, dict and `in`;
the complement is the oracle's table (recruit_sets.revcomp).

A designed token carries the verdict it was designed for — joins the group of token X, founds a group, dropped, survives — and
the builder asserts its own premises (which earlier token owns each of a token's 11-mers, in position order), so that a set
cannot drift away from what its name says.  test_merge_sets_host.py checks every verdict against the reference, the reference
against the oracle and the host merge, before test_gpu_merge_sets.py trusts either.  Everything is deterministic (fixed seeds)."""
import random

from tests import recruit_sets as rs

KMER = 11                                              # CRASS_DEF_KMER_SIZE
_COMP = bytes(rs.revcomp(bytes([b]))[0] for b in range(256))


def revcomp(s):
    """reverseComplement by the oracle's table, one byte at a time (recruit_sets.revcomp)"""
    return bytes(s).translate(_COMP)[::-1]


def laurenize(kmer):
    rc = revcomp(kmer)
    return kmer if kmer < rc else rc


def kmers(tok):
    return [laurenize(tok[i:i + KMER]) for i in range(len(tok) - KMER + 1)]


def dedupe(rows):
    """first-occurrence order: the StringCheck token order"""
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def merge_reference(tokens, kmer_clust_size):
    """(groups, patterns, pat_group, dropped) of distinct strings in token order.
    groups: per GID 1, 2, ... the member tokens' ids (index + 2) ascending; patterns: per group the survivors by (length, token),
    then their reverse complements; pat_group: the GID of every pattern; dropped: the set of token indices removed as redundant."""
    tokens = [bytes(t) for t in tokens]
    assert len(set(tokens)) == len(tokens)
    k2gid, gid, next_gid = {}, [], 1
    for tok in tokens:                                 # clusterDRReads, in token order
        assert len(tok) >= KMER
        count, homeless, group = {}, [], 0
        for km in kmers(tok):
            if km not in k2gid:
                homeless.append(km)
            elif group == 0:
                g = k2gid[km]
                if g not in count:
                    count[g] = 1                       # a first sighting is not compared with the threshold
                else:
                    count[g] += 1
                    if kmer_clust_size <= count[g]:
                        group = g
        if group == 0:
            group = next_gid
            next_gid += 1
        for km in homeless:
            k2gid[km] = group
        gid.append(group)
    groups = [[t + 2 for t in range(len(tokens)) if gid[t] == g] for g in range(1, next_gid)]
    patterns, pat_group, dropped = [], [], set()
    for g, members in enumerate(groups, 1):            # removeRedundantRepeats per group
        order = sorted((t - 2 for t in members), key=lambda t: (len(tokens[t]), t))
        blank = set()
        for i, a in enumerate(order):
            if a in blank:
                continue
            rc = revcomp(tokens[a])
            # (no length check, as in the reference and the oracle: an equal-length member is blanked when it IS rc(a).  The device
            # compares strictly shorter members only.  The two cannot differ on tokens pass 1 makes — a token is the low-lexi form of
            # its repeat, so a and rc(a) are never both tokens — and TokenSet.add keeps the designed sets inside that domain.)
            for b in order[i + 1:]:
                if b not in blank and (tokens[a] in tokens[b] or rc in tokens[b]):
                    blank.add(b)
        kept = [tokens[t] for t in order if t not in blank]
        patterns += kept + [revcomp(p) for p in kept]
        pat_group += [g] * (2 * len(kept))
        dropped |= blank
    return groups, patterns, pat_group, dropped


# ---- designed token sets ----
def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choices(alphabet, k=n))


def _other(rng, b):
    return bytes([rng.choice([x for x in b"ACGT" if x != b])])


def low_lexi(tok):
    """a token is the DRLowLexi form of its repeat, as pass 1 makes it: smaller than its reverse complement"""
    return tok < revcomp(tok)


def _rand_low(rng, n):
    """a random low-lexi token"""
    while True:
        tok = _rand(rng, n)
        if low_lexi(tok):
            return tok


def _needle(rng, n):
    """a random token A ... C|G: low-lexi, and so is a haystack that starts with it, or with its reverse complement (C|G ...)
    where the haystack ends in A"""
    return b"A" + _rand(rng, n - 2) + bytes([rng.choice(b"CG")])


class TokenSet:
    """tokens in order, per class the designed tokens, per designed token its verdict: a dict with 'joins' (token index), 'founds'
    (True) and / or 'dropped' (True: removed as redundant, False: survives)"""

    def __init__(self, name, k, seed, low=23, high=47, lens=None):
        self.name, self.k, self.thr = name, k, max(k, 2)
        self.low, self.high = low, high
        self.stride = (high + 15) & ~15
        self.lens = list(lens or range(low, high + 1))
        self.rng = random.Random(seed)
        self.tokens, self.classes, self.verdict = [], {}, {}
        self.owner = {}                                # laurenized 11-mer -> the first token that holds it
        self.read_tokens = []                          # tokens whose patterns the designed reads are made of, beside the sampled ones
        self.run = None                                # T*16 / A*16 where the set is about that anchor key: extra reads (_design)

    def params(self):
        return dict(lowDRsize=self.low, highDRsize=self.high, kmer_clust_size=self.k)

    def sightings(self, tok):
        """owners of the token's 11-mers that an earlier token holds, in position order (one entry per occurrence)"""
        return [self.owner[km] for km in kmers(tok) if km in self.owner]

    def root(self, t):
        """the founder of the group token t was designed into"""
        while "joins" in self.verdict[t]:
            t = self.verdict[t]["joins"]
        return t

    def length(self, need):
        ok = [x for x in self.lens if x >= need]
        assert ok, (self.name, need)
        return self.rng.choice(ok)

    def add(self, cls, tok, joins=None, founds=False, dropped=None, expect=None, reads=False):
        tok = bytes(tok)
        assert self.low <= len(tok) <= self.high, (cls, len(tok))
        assert tok not in self.tokens and revcomp(tok) not in self.tokens, cls
        assert low_lexi(tok), (cls, tok)
        if expect is not None:
            assert self.sightings(tok) == expect, (cls, self.sightings(tok), expect)
        t = len(self.tokens)
        self.tokens.append(tok)
        for km in kmers(tok):
            self.owner.setdefault(km, t)
        v = {}
        if joins is not None:
            v["joins"] = joins
        if founds:
            v["founds"] = True
        if dropped is not None:
            v["dropped"] = dropped
        assert v, cls
        self.classes.setdefault(cls, []).append(t)
        self.verdict[t] = v
        if reads:
            self.read_tokens.append(t)
        return t

    def splice(self, parts, expect, total=None, left=0, right=0):
        """random tail + parts + random tail of `total` bases (left / right: the tails' least lengths) whose sightings are exactly
        `expect`: the tails and the junctions add none.  parts: a list, or a function that draws one (tried again with the tails)"""
        draw = parts if callable(parts) else (lambda: parts)
        n_body = len(b"".join(draw()))
        total = total or self.length(max(self.low, n_body + left + right))
        spare = total - n_body - left - right
        assert spare >= 0, (self.name, total, n_body)
        for _ in range(400):
            body = b"".join(draw())
            assert len(body) == n_body
            a = self.rng.randint(0, spare)
            tok = _rand(self.rng, left + a) + body + _rand(self.rng, right + spare - a)
            if self.sightings(tok) == expect and tok not in self.tokens and low_lexi(tok):
                return tok
        raise AssertionError((self.name, "no tails found", expect))

    def founder(self, cls="founder", n=None, **kw):
        tok = _rand_low(self.rng, n or self.length(max(self.low, 2 * self.thr + 10)))
        return self.add(cls, tok, founds=True, expect=[], **kw)

    def seg(self, t, n_kmers, at=None, rc=False):
        """n_kmers consecutive 11-mers of token t (from position `at`, else a random one), forward or reverse-complemented"""
        tok = self.tokens[t]
        n = n_kmers + KMER - 1
        assert n <= len(tok), (self.name, n, len(tok))
        a = self.rng.randint(0, len(tok) - n) if at is None else at
        s = tok[a:a + n]
        return revcomp(s) if rc else s


def _threshold_family(ts, f, tag=""):
    thr = ts.thr
    for s in (thr - 1, thr, thr + 1):
        for rc in (False, True):
            if s + KMER - 1 > len(ts.tokens[f]):
                continue
            tok = ts.splice([ts.seg(f, s, rc=rc)], [f] * s, left=0 if s + KMER - 1 == ts.high else 1)
            cls = "threshold%s_%s_%s" % (tag, {thr - 1: "minus1", thr: "exact", thr + 1: "plus1"}[s], "rc" if rc else "fwd")
            ts.add(cls, tok, expect=[f] * s, **({"joins": f} if s >= thr else {"founds": True}))


def _cluster_families(ts):
    thr, hi = ts.thr, ts.high
    # threshold - 1 | threshold | threshold + 1 shared 11-mers, forward and through the reverse complement
    _threshold_family(ts, ts.founder())
    # first to reach the threshold along the token wins: not the group seen first, not the lowest GID, not the largest count
    a, b = ts.founder(n=ts.length(3 * thr + 10)), ts.founder(n=ts.length(3 * thr + 10))
    n2 = 2 * thr if 3 * thr + 20 <= hi else thr
    ts.add("chimera_later_group_first", ts.splice(lambda: [ts.seg(b, thr), ts.seg(a, n2)], [b] * thr + [a] * n2), joins=b)
    ts.add("chimera_earlier_group_first", ts.splice(lambda: [ts.seg(a, thr), ts.seg(b, n2)], [a] * thr + [b] * n2), joins=a)
    if 2 * thr + 30 <= hi:
        def parts():
            return [ts.seg(a, thr - 1, at=0), ts.seg(b, thr), ts.seg(a, 1, at=len(ts.tokens[a]) - KMER)]
        ts.add("chimera_seen_first_loses", ts.splice(parts, [a] * (thr - 1) + [b] * thr + [a]), joins=b)
    # sightings add up across the owner tokens of one group
    t1 = ts.founder()
    t2 = ts.add("addup_brings_kmers", ts.splice([ts.seg(t1, thr + 1)], [t1] * (thr + 1), left=thr), joins=t1)
    ts.add("addup_only_new_kmers", ts.splice([ts.tokens[t2][:thr + KMER - 1]], [t2] * thr, right=1), joins=t1)
    ts.add("addup_two_owners", ts.splice(lambda: [ts.seg(t1, thr - 1), ts.tokens[t2][:KMER]], [t1] * (thr - 1) + [t2]), joins=t1)
    # under the threshold: a group of its own, which a later token joins through the new 11-mers
    v = ts.add("below_threshold_founds", ts.splice([ts.seg(t1, thr - 1)], [t1] * (thr - 1), left=thr), founds=True)
    ts.add("joins_the_new_group", ts.splice([ts.tokens[v][:thr + KMER - 1]], [v] * thr, right=1), joins=v)
    # a homopolymer run: one 11-mer at every position of the run
    tok = ts.splice(lambda: [_other(ts.rng, ord("A")) + b"A" * 13 + _other(ts.rng, ord("A"))], [])
    ts.add("homopolymer_first_holder", tok, founds=True)                     # its own repeats are not sightings
    o = ts.add("homopolymer_owner", ts.splice([b"A" + b"C" * 11 + b"G"], []), founds=True)
    ts.add("homopolymer_run13", ts.splice([b"T" + b"C" * 13 + b"T"], [o] * 3), **({"joins": o} if thr <= 3 else {"founds": True}))
    ts.add("homopolymer_run_reaches", ts.splice([b"G" + b"C" * (thr + 10) + b"A"], [o] * thr), joins=o)


def cluster(k):
    ts = TokenSet("cluster", k, "cluster %d" % k)
    _cluster_families(ts)
    # tokens of exactly 23 and 47 bases: founders and their variants
    for n in (23, 47):
        f = ts.founder("founder_%d" % n, n=n)
        for s in (ts.thr - 1, ts.thr):
            tok = ts.splice([ts.seg(f, s)], [f] * s, total=n)
            ts.add("exact_%d_%s" % (n, "joins" if s >= ts.thr else "founds"), tok, **({"joins": f} if s >= ts.thr else {"founds": True}))
    return ts


WIDE_LENS = (48, 54, 55, 63, 64)


def cluster_wide(k):
    """highDRsize = 64 (stride 64): every token is 48, 54, 55, 63 or 64 bases; a 64-base token has 54 11-mers and uses base 63"""
    ts = TokenSet("cluster_wide", k, "cluster wide %d" % k, high=64, lens=WIDE_LENS)
    _cluster_families(ts)
    f = ts.founder("founder_64", n=64)
    _threshold_family(ts, f, "64")
    # the last 11-mers of a 64-base founder (positions 43 .. 53, bases up to 63), shared with 64-base variants
    s = ts.thr
    ts.add("last_kmers_64", ts.splice([ts.seg(f, s, at=54 - s)], [f] * s, total=64, right=0), joins=f)
    ts.add("last_kmers_64_minus1", ts.splice([ts.seg(f, s - 1, at=55 - s)], [f] * (s - 1), total=64), founds=True)
    assert {len(t) for t in ts.tokens} == set(WIDE_LENS)
    return ts


def _same_group_pair(ts, needle, hay, cls, dropped, **kw):
    """a haystack built around a needle's bases (hay: bytes, or a function that draws them — random tails — until the premise
    holds): every 11-mer it shares is owned by the needle's group (by design) and there are at least thr, so it joins that group"""
    for _ in range(200):
        h = hay() if callable(hay) else hay
        n = [ts.root(o) for o in ts.sightings(h)]
        if n.count(ts.root(needle)) >= ts.thr and set(n) == {ts.root(needle)} and (low_lexi(h) or not callable(hay)):
            return ts.add(cls, h, joins=needle, dropped=dropped, **kw)
        assert callable(hay), (cls, n)
    raise AssertionError((cls, "no tails found"))


def redundant():
    ts = TokenSet("redundant", 6, "redundant")
    rng = ts.rng
    # a needle at offset 0, in the middle, at the last offset; forward and as its reverse complement
    n = ts.add("needle", _needle(rng, 25), founds=True, dropped=False, expect=[], reads=True)
    nd = ts.tokens[n]
    for tag, s in (("fwd", nd), ("rc", revcomp(nd))):
        _same_group_pair(ts, n, lambda: s + _rand(rng, 15), "needle_offset0_" + tag, True)
        _same_group_pair(ts, n, lambda: _rand(rng, 7) + s + _rand(rng, 8), "needle_middle_" + tag, True)
        _same_group_pair(ts, n, lambda: _rand(rng, 22) + s, "needle_last_offset_" + tag, True)
    # one base shorter than the haystack
    _same_group_pair(ts, n, lambda: nd + _rand(rng, 1), "one_shorter_offset0", True)
    _same_group_pair(ts, n, lambda: _rand(rng, 1) + nd, "one_shorter_offset1", True)
    # equal lengths, one base apart: both survive
    e = ts.add("equal_length", _needle(rng, 30), founds=True, dropped=False, expect=[], reads=True)
    q = bytearray(ts.tokens[e])
    q[29] = ord("C") + ord("G") - q[29]                # (C | G: still low-lexi)
    _same_group_pair(ts, e, bytes(q), "equal_length_one_base", False, reads=True)
    # near misses: a window with the needle's first 16 bases, a mismatch at base 17 or at the needle's last base
    m = ts.add("near_miss_needle", _needle(rng, 27), founds=True, dropped=False, expect=[], reads=True)
    for at, tag in ((16, "base17"), (26, "last_base")):
        for rc in (False, True):
            q = bytearray(ts.tokens[m])
            q[at] = _other(rng, q[at])[0]
            s = revcomp(bytes(q)) if rc else bytes(q)
            _same_group_pair(ts, m, lambda: _rand(rng, 5) + s + _rand(rng, 6), "near_miss_%s_%s" % (tag, "rc" if rc else "fwd"), False, reads=not rc)
    # a chain A in B in C, the link A -> B through the reverse complement
    a = ts.add("chain_a", _needle(rng, 24), founds=True, dropped=False, expect=[], reads=True)
    b = _same_group_pair(ts, a, lambda: _rand(rng, 4) + revcomp(ts.tokens[a]) + _rand(rng, 5), "chain_b", True)
    _same_group_pair(ts, a, lambda: _rand(rng, 6) + ts.tokens[b] + _rand(rng, 3), "chain_c", True)
    # a haystack in front of its needle in token order: the needle joins the haystack's group, the haystack is dropped all the same
    h = ts.add("haystack_first", _rand_low(rng, 44), founds=True, dropped=True, expect=[])
    at = min(o for o in range(1, 18) if low_lexi(ts.tokens[h][o:o + 26]))
    ts.add("needle_second", ts.tokens[h][at:at + 26], joins=h, dropped=False, reads=True)
    # 70 needles of one group whose first 22 bases are equal: one key of the needle index, two rounds of 64 candidates
    head = b"A" + _rand(rng, 21)
    needles = []
    for i in range(70):
        tok = head + _rand(rng, 7) + bytes([rng.choice(b"CG")])
        if i == 0:
            needles.append(ts.add("many_needles", tok, founds=True, dropped=False, expect=[], reads=True))
        else:
            needles.append(ts.add("many_needles", tok, joins=needles[0], dropped=False, reads=i in (1, 35, 69)))
    for i in (0, 1, 33, 63, 64, 69):
        _same_group_pair(ts, needles[0], lambda: _rand(rng, 9) + ts.tokens[needles[i]] + _rand(rng, 8), "many_needles_haystack", True)
    for _ in range(2):
        h = _same_group_pair(ts, needles[0], lambda: _rand(rng, 9) + head + _rand(rng, 16), "many_needles_no_needle", False, reads=True)
        assert not any(ts.tokens[x] in ts.tokens[h] for x in needles)
    return ts


def redundant_k20():
    """kmer_clust_size = 20: a 25-base token (15 11-mers) and a longer token that holds it stay in different groups, nothing is
    dropped, and both become patterns that end at the same base of a read: the longest is reported"""
    ts = TokenSet("redundant_k20", 20, "redundant k20")
    rng = ts.rng
    for n_pre in (12, 20):
        x = ts.add("short_token", _needle(rng, 25), founds=True, dropped=False, expect=[], reads=True)
        tok = ts.splice([ts.tokens[x]], [x] * 15, total=n_pre + 25, left=n_pre)
        ts.add("longer_holds_it", tok, founds=True, dropped=False, expect=[x] * 15, reads=True)
    while True:
        tok = _rand_low(rng, 47)
        if low_lexi(tok[-25:]):
            break
    y = ts.add("longer_first", tok, founds=True, dropped=False, expect=[], reads=True)
    ts.add("short_second", ts.tokens[y][-25:], founds=True, dropped=False, expect=[y] * 15, reads=True)
    return ts


def second_batch_window(hay_len, rc_offset, low=23):
    """the number of the window in which k_dm_redundant finds a needle at rc_offset of the haystack's reverse complement: the
    windows are numbered orientation * nwin + offset, nwin = hay_len - low + 1, 64 per round"""
    return (hay_len - low + 1) + rc_offset


def redundant_wide():
    """stride 64: haystacks of 55 .. 64 bases whose needle is found only in a window of the second round of 64 — the
    reverse-complement orientation at a late offset"""
    ts = TokenSet("redundant_wide", 6, "redundant wide", high=64)
    rng = ts.rng
    for n in range(55, 65):
        nd_len = 23 + (n % 3)
        nd = ts.add("needle", _needle(rng, nd_len), founds=True, dropped=False, expect=[], reads=n in (55, 64))
        s = revcomp(ts.tokens[nd])
        # rc(needle) at offset 0 <=> the needle at the last offset of rc(haystack)
        h = _same_group_pair(ts, nd, lambda: s + _rand(rng, n - nd_len), "second_batch_%d" % n, True)
        hay = ts.tokens[h]
        assert ts.tokens[nd] not in hay and revcomp(hay).find(ts.tokens[nd]) == n - nd_len
        assert second_batch_window(n, n - nd_len) >= 64
        q = bytearray(s)
        q[2] = _other(rng, q[2])[0]                    # the needle's base nd_len - 3: behind the 16 bases of the window's key
        q = bytes(q)
        _same_group_pair(ts, nd, lambda: q + _rand(rng, n - nd_len), "second_batch_miss_%d" % n, False, reads=n in (55, 64))
    # a needle of 63 bases in a haystack of 64, both ends
    nd = ts.add("needle_63", _needle(rng, 63), founds=True, dropped=False, expect=[], reads=True)
    _same_group_pair(ts, nd, lambda: ts.tokens[nd] + _rand(rng, 1), "one_shorter_64_offset0", True)
    _same_group_pair(ts, nd, lambda: revcomp(ts.tokens[nd]) + _rand(rng, 1), "one_shorter_64_offset1_rc", True)
    return ts


def _laurenize_n_as_a(kmer):
    """the wrong rule an 'N' packed as 'A' would give: compare with N read as A"""
    rc = revcomp(kmer)
    return kmer if kmer.replace(b"N", b"A") < rc.replace(b"N", b"A") else rc


def n_mask(wide=False):
    ts = TokenSet("n_mask_wide" if wide else "n_mask", 6, "n mask %d" % wide, high=64 if wide else 47)
    rng = ts.rng

    def with_n(n, at):
        q = bytearray(_needle(rng, n))
        q[at] = ord("N")
        return bytes(q)

    def swap(tok, at, ch):
        q = bytearray(tok)
        q[at] = ch
        return bytes(q)
    cases = [(36, 30, 4, 5), (40, 35, 3, 4)] + ([(56, 50, 4, 4), (58, 57, 6, 0)] if wide else [])
    for n, at, pre, post in cases:
        tag = "n_at_%d" % at
        for rc in (False, True):
            o = "rc" if rc else "fwd"
            f = (lambda s: revcomp(s)) if rc else (lambda s: s)
            if rc:
                pre, post = post, pre                  # (the N keeps its distance from the haystack's end in that orientation)
            nn = ts.add("needle_with_n_%s_%s" % (tag, o), with_n(n, at), founds=True, dropped=False, expect=[], reads=not rc)
            tok = ts.tokens[nn]
            _same_group_pair(ts, nn, lambda: _rand(rng, pre) + f(tok) + _rand(rng, post), "n_on_n_%s_%s" % (tag, o), True)
            _same_group_pair(ts, nn, lambda: _rand(rng, pre) + f(swap(tok, at, ord("A"))) + _rand(rng, post), "n_needle_a_haystack_%s_%s" % (tag, o), False)
            na = ts.add("needle_with_a_%s_%s" % (tag, o), swap(with_n(n, at), at, ord("A")), founds=True, dropped=False, expect=[])
            tok = ts.tokens[na]
            _same_group_pair(ts, na, lambda: _rand(rng, pre) + f(swap(tok, at, ord("N"))) + _rand(rng, post), "a_needle_n_haystack_%s_%s" % (tag, o), False)
    if wide:
        # N at base 63 of a 64-base haystack, aligned with the N at the needle's last base
        nn = ts.add("needle_n_last_base", with_n(41, 40), founds=True, dropped=False, expect=[])
        tok = ts.tokens[nn]
        h = _same_group_pair(ts, nn, lambda: _rand(rng, 23) + tok, "n_at_base_63", True)
        assert ts.tokens[h][63] == ord("N")
        _same_group_pair(ts, nn, lambda: _rand(rng, 23) + swap(tok, 40, ord("A")), "a_at_base_63", False)
        nr = ts.add("needle_n_first_base", b"N" + _rand(rng, 39) + b"A", founds=True, dropped=False, expect=[])
        h = _same_group_pair(ts, nr, lambda: _rand(rng, 23) + revcomp(ts.tokens[nr]), "n_at_base_63_rc", True)
        assert ts.tokens[h][63] == ord("N")
    # 11-mers that hold the N, shared through the reverse complement: thr of them join, thr - 1 do not; at least one of them
    # laurenizes differently when the N is read as A
    thr = ts.thr
    for _ in range(200):
        f = with_n(34, 17)
        shared = [f[i:i + KMER] for i in range(17 - 8, 17 - 8 + thr)]
        if any(laurenize(km) != _laurenize_n_as_a(km) for km in shared):
            break
    else:
        raise AssertionError("no N 11-mer whose laurenized form depends on the order of N")
    fn = ts.add("n_kmer_founder", f, founds=True, dropped=False, expect=[])
    assert all(b"N" in km for km in shared)
    ts.add("n_kmers_join_rc", ts.splice([revcomp(f[9:9 + thr + 10])], [fn] * thr, left=1, right=1), joins=fn)
    ts.add("n_kmers_below_rc", ts.splice([revcomp(f[9:9 + thr + 9])], [fn] * (thr - 1), left=1, right=1), founds=True)
    ts.add("n_kmers_join_fwd", ts.splice([f[9:9 + thr + 10]], [fn] * thr, left=1, right=1), joins=fn)
    return ts


def short_keys(k):
    """lowDRsize = 15, highDRsize = 37: tokens of 15 .. 18 bases (needle and window keys cut to 15 bases, anchor keys every 4
    bases), a 15-base needle at the last offset, the threshold family"""
    ts = TokenSet("short_keys", k, "short keys %d" % k, low=15, high=37)
    rng, thr = ts.rng, ts.thr
    _threshold_family(ts, ts.founder(n=37))
    for n in (15, 16, 17, 18):
        ts.add("short_token_%d" % n, _needle(rng, n), founds=True, dropped=False, expect=[], reads=True)
    # a 15-base needle (five 11-mers) at the last offset of haystacks of 16 .. 37 bases: dropped where the two share a group
    for n in (16, 18, 19, 30, 37):
        nd = ts.add("needle_15", _needle(rng, 15), founds=True, dropped=False, expect=[], reads=n in (16, 37))
        hay = ts.splice([ts.tokens[nd]], [nd] * 5, total=n, left=n - 15)
        same = 5 >= thr
        ts.add("needle_15_last_offset_%d" % n, hay, expect=[nd] * 5, dropped=same, **({"joins": nd} if same else {"founds": True}), reads=not same and n == 37)
        if n >= 18:
            hay = ts.splice([revcomp(ts.tokens[nd])], [nd] * 5, total=n, right=n - 15)
            ts.add("needle_15_rc_offset0_%d" % n, hay, expect=[nd] * 5, dropped=same, **({"joins": nd} if same else {"founds": True}))
    return ts


def t_run_token(rng, at, n):
    """n bases with T*16 at offset `at` (and no seventeenth T), as the low-lexi form: the pattern list holds both orientations"""
    tail = _other(rng, ord("T")) + _rand(rng, n - at - 17)
    head = _rand(rng, at - 1) + _other(rng, ord("T")) if at else b""
    tok = head + b"T" * 16 + tail
    assert len(tok) == n and tok.find(b"T" * 16) == at and b"T" * 17 not in tok
    return min(tok, revcomp(tok))


T_OFF8_SEED = "all t off 8 0"       # (chosen so that the set's one-slot keys leave every key of the GPU cases a slot: unplaceable_keys)


def all_t(off8=False, low=23):
    """surviving tokens with T*16 at pattern offsets 0 and 7: the 16-mer there is the anchor key 0xFFFFFFFF, the cuckoo table's
    free-slot mark.  off8: the run at offset 8 only — no such key, and the reverse complement (28 bases) holds A*16 = key 0.
    low = 19: lowDRsize 19 — 16-base keys at offsets 0 .. 3 only (windows every 4 bases), beside tokens of 19 .. 22 bases"""
    ts = TokenSet("t_off8" if off8 else "all_t", 6, T_OFF8_SEED if off8 else "all t", low=low)
    ts.run = b"A" * 16 if off8 else b"T" * 16
    rng = ts.rng
    for i, (at, n) in enumerate(((0, 28), (7, 35), (0, 40), (7, 47))):
        tok = t_run_token(rng, 8, 28) if off8 else t_run_token(rng, at, n)
        v = dict(dropped=False, reads=True)
        if i == 0:
            ts.add("t_run", tok, founds=True, expect=[], **v)
        else:
            ts.add("t_run", tok, joins=0, **v)            # (the run's 11-mer, six times: the threshold of 6 is reached)
    for _ in range(6):
        ts.add("plain", _rand_low(rng, rng.randint(23, 47)), founds=True, dropped=False, expect=[], reads=True)
    for n in (19, 20, 22) if low == 19 else ():
        ts.add("short_token_%d" % n, _needle(rng, n), founds=True, dropped=False, expect=[], reads=True)
    keys = anchor_key_strings([p for t in ts.tokens for p in (t, revcomp(t))], low)
    assert (b"T" * 16 in keys) == (not off8) and (b"A" * 16 in keys) == off8
    return ts


def anchor_shape(low):
    """(bases per anchor key, key offsets per pattern) for a job's lowDRsize — the rule key + alignment - 1 <= lowDRsize with keys
    of 16 | 12 bases and windows every 8 | 4 bases: from 23 on 16-base keys at offsets 0 .. 7, 19 .. 22: 16-base keys at 0 .. 3,
    15 .. 18: 12-base keys at 0 .. 3"""
    assert low >= 15
    return (16 if low >= 19 else 12), (8 if low >= 23 else 4)


def anchor_key_strings(patterns, low=23):
    """the distinct anchor keys of a pattern list as the device takes them: every pattern, an N read as the A it is packed as (the
    mask bit is the verification's business, not the filter's).  Without an N and from lowDRsize 23 on their number is
    recruit_sets.anchor_keys'"""
    kl, n_off = anchor_shape(low)
    assert all(len(p) >= kl + n_off - 1 for p in patterns)
    return {p.replace(b"N", b"A")[r:r + kl] for p in patterns for r in range(n_off)}


# The device's anchor table is a two-choice cuckoo table over the 16-mers' 2-bit values (base i in bits 2i, 2i + 1; A C G T =
# 0 1 2 3), slot_i(V) = ak_hash(V, m_i) >> (32 - log), log = 10 while 3 * keys <= 1 024.  0xFFFFFFFF — T*16 — marks a free slot
# and is never inserted: a window of T*16 is found through a FREE slot among its two.  all_t_blocked puts other keys there.
AK_M = (0x9E3779, 0x85EBCB)


def ak_hash(v, m):
    return ((v & 0xFFFFFF) * m + (v & 0xFF000000)) & 0xFFFFFFFF


def key_value(p16):
    return sum(b"ACGT".index(b) << (2 * i) for i, b in enumerate(p16))


BLOCK_BITS = 12                                        # the blocking keys share the all-T key's slot for every log up to this


def all_t_blocked():
    """all_t, and two more tokens whose first 16 bases are keys whose FIRST slot is the all-T key's first and second slot: both
    slots of T*16 are then taken whatever the insertion order (a key takes its first slot when it is free, and a taken slot
    never becomes free), for tables of 2^10 .. 2^12 slots"""
    ts = all_t()
    ts.name = "all_t_blocked"
    rng = random.Random("all t blocked")
    for i, m in enumerate(AK_M):
        slot = ak_hash(0xFFFFFFFF, m) >> (32 - BLOCK_BITS)
        while True:
            k16 = b"A" + _rand(rng, 15)
            if ak_hash(key_value(k16), AK_M[0]) >> (32 - BLOCK_BITS) == slot:
                break
        tok = k16 + _rand(rng, 10) + bytes([rng.choice(b"CG")])
        assert low_lexi(tok) and key_value(tok[:16]) != 0xFFFFFFFF
        ts.add("blocks_slot_%d" % (i + 1), tok, founds=True, dropped=False, expect=[], reads=True)
    return ts


def blocked_slots(patterns, log):
    """of the all-T key's two slots in a table of 2^log slots, those that are the first slot of another key of the patterns"""
    first = {ak_hash(key_value(p[r:r + 16]), AK_M[0]) >> (32 - log) for p in patterns if not set(p) - set(b"ACGT") for r in range(8)
             if p[r:r + 16] != b"T" * 16}
    return [ak_hash(0xFFFFFFFF, m) >> (32 - log) in first for m in AK_M]


def table_log(n_keys):
    """log2 of the device table's slots for a key count (dm_table_params: load <= 1/3, <= 1/2 at 2^15 and at 2^16)"""
    for log in range(10, 16):
        if n_keys * 3 <= 1 << log or (log == 15 and n_keys * 2 <= 1 << log):
            return log
    if n_keys * 2 <= 1 << 16:
        return 16
    return min(log for log in range(17, 25) if n_keys * 3 <= 1 << log)


def unplaceable_keys(patterns, low=23):
    """the anchor keys of a pattern list that NO two-choice placement with the device's one hash pair can hold (a maximum
    matching of keys to slots): the device merge then gives up and the host merges — correctly, but it is not the device's tables
    that pass 2 runs over.  A key whose low 24 bits are zero (twelve A's first) has one slot, not two: sets with A*16 make several.
    With the all-T key among them its first slot is nobody else's."""
    import sys
    keys = sorted(key_value(k) for k in anchor_key_strings(patterns, low))
    log = table_log(len(keys))
    all_t = 0xFFFFFFFF in keys
    keep = ak_hash(0xFFFFFFFF, AK_M[0]) >> (32 - log) if all_t else -1
    slots = {k: {ak_hash(k, m) >> (32 - log) for m in AK_M} - {keep} for k in keys if k != 0xFFFFFFFF}
    match = {}
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))

    def place(k, seen):
        for s in slots[k]:
            if s not in seen:
                seen.add(s)
                if s not in match or place(match[s], seen):
                    match[s] = k
                    return True
        return False
    return [k for k in slots if not place(k, set())]


TIER_TOKENS = (900, 1800, 3400)
TIER_KEYS = ((0, 16384), (16384, 32768), (32768, 1 << 30))         # dm_table_params: exact keys in LDS | 2^16 slots | probed in L2
TIER_MARGIN = 1500                                                 # room for the keys of the context's own tokens


def tiers(i):
    ts = TokenSet("tiers%d" % i, 6, "tiers")
    ts.run = b"T" * 16
    for j in range(TIER_TOKENS[i]):
        ts.add("unrelated", _rand_low(ts.rng, ts.rng.randint(23, 47)), founds=True, dropped=False, reads=j % 300 == 7)
        if j == 500:                                   # the all-T key in every tier's table form: at a pattern's offset 0 | 0 | 7
            ts.add("t_run", t_run_token(ts.rng, (0, 0, 7)[i], 30 + i), founds=True, dropped=False, reads=True)
    n = rs.anchor_keys([p for t in ts.tokens for p in (t, revcomp(t))])
    assert TIER_KEYS[i][0] + TIER_MARGIN < n <= TIER_KEYS[i][1] - TIER_MARGIN, n
    return ts


def declined(form):
    """a valid set and one token the device merge does not take: 22 bases (under lowDRsize), or a base outside ACGTN"""
    ts = TokenSet("declined_" + form, 6, "declined")
    f = ts.founder()
    _threshold_family(ts, f)
    assert min(len(t) for t in ts.tokens) >= 23
    if form == "short":
        ts.low = 22                                    # (for this one token)
        ts.add("token_22", _rand_low(ts.rng, 22), founds=True, dropped=False, expect=[])
    else:
        q = bytearray(_needle(ts.rng, 30))
        q[11] = ord("R")
        ts.add("token_with_r", bytes(q), founds=True, dropped=False, expect=[])
    ts.low = 23                                        # the engine's parameters stay the default ones
    return ts


_SETS = {}
SET_NAMES = ["cluster-%d" % k for k in (1, 2, 6, 12)] + ["cluster_wide-%d" % k for k in (1, 2, 6, 12)] + \
            ["redundant", "redundant_k20", "redundant_wide", "n_mask", "n_mask_wide", "short_keys-2", "short_keys-6", "all_t", "t_off8", "all_t_blocked", "all_t_low19",
             "tiers0", "tiers1", "tiers2", "declined_short", "declined_r"]


def token_set(name):
    if name not in _SETS:
        base, _, k = name.partition("-")
        make = {"cluster": cluster, "cluster_wide": cluster_wide, "short_keys": short_keys}
        if base in make:
            ts = make[base](int(k))
        else:
            ts = {"redundant": redundant, "redundant_k20": redundant_k20, "redundant_wide": redundant_wide, "n_mask": n_mask,
                  "n_mask_wide": lambda: n_mask(True), "all_t": all_t, "t_off8": lambda: all_t(True), "all_t_blocked": all_t_blocked, "all_t_low19": lambda: all_t(low=19),
                  "tiers0": lambda: tiers(0), "tiers1": lambda: tiers(1), "tiers2": lambda: tiers(2),
                  "declined_short": lambda: declined("short"), "declined_r": lambda: declined("r")}[base]()
        ts.name = name
        ts.reference = merge_reference(ts.tokens, ts.k)
        _SETS[name] = ts
    return _SETS[name]


# ---- designed pass-2 reads over the reference's patterns ----
LAYOUTS = ("u150", "u184", "u304", "u320", "ragged")   # k_dm_verify: three reads per wave | one read per wave, words in LDS (two
                                                       # lengths) | beyond DV_MAXW = 20 words: global loads | per-read lengths
# every set on 150-base reads; the sets whose patterns ask something of the verification (ties, N — at base 63 too —, the all-T
# key, 64-base patterns, short keys, a full LDS table) on every layout
READ_LAYOUT_SETS = ("redundant", "redundant_k20", "redundant_wide", "n_mask", "n_mask_wide", "all_t", "t_off8", "all_t_blocked", "all_t_low19",
                    "cluster_wide-6", "short_keys-2", "tiers0")
READ_CASES = [(n, "u150") for n in SET_NAMES] + [(n, lay) for n in READ_LAYOUT_SETS for lay in LAYOUTS[1:]]
N_READS = {"u150": 2003, "u184": 1203, "u304": 1203, "u320": 1203, "ragged": 2003}


def read_core(ts):
    """the surviving patterns the designed reads are made of, by name: 'full' patterns take every class of recruit_sets.design,
    'plain' ones (a pattern inside or around another pattern, or with an N) only the classes whose verdict is 'recruited'"""
    groups, patterns, pat_group, dropped = ts.reference
    pset = set(patterns)
    picked = [t for t in ts.read_tokens if t not in dropped]
    rest = [t for t in sorted(ts.verdict) if t not in dropped and t not in picked]
    random.Random("core " + ts.name).shuffle(rest)
    picked += rest[:max(0, 10 - len(picked))]
    full, plain = {}, {}
    for t in picked:
        for tag, p in (("t%d" % t, ts.tokens[t]), ("t%drc" % t, revcomp(ts.tokens[t]))):
            assert p in pset
            if len(p) < 23 or set(p) - set(b"ACGT") or any(q != p and (q in p or p[:-1] in q or p[1:] in q) for q in patterns):
                plain[tag] = p
            else:
                full[tag] = p
    return full, plain


def _design(c, ts, L, rng):
    full, plain = read_core(ts)
    for tag, p in full.items():
        rs.design(c, {tag: p}, L, rng, exc=False, classes=("window_start", "window_end", "cut", "start16"))
        n = len(p)
        for o in (0, 1, 7, 8, 9):                      # one base changed, behind and inside the first key
            if o + n <= L:
                for at in (n - 1, 20, 3):
                    q = bytearray(p)
                    q[at] = _other(rng, q[at])[0]
                    c.add("near_miss", rs._place(rng, L, o, bytes(q)), False)
    for tag, p in plain.items():
        rs.design(c, {tag: p}, L, rng, exc=False, classes=("window_start", "window_end", "start16"))
        if b"N" in p and len(p) <= L:
            for o in (0, (L - len(p)) // 2, L - len(p)):
                c.add("n_pattern_as_is", rs._place(rng, L, o, p), True)
                if not any(q in p.replace(b"N", b"A") for q in c.patterns):        # (a haystack that held the needle but for its N)
                    c.add("n_pattern_a_for_n", rs._place(rng, L, o, p.replace(b"N", b"A")), False)
                c.add("n_pattern_r_for_n", rs._place(rng, L, o, p.replace(b"N", b"R")), False)
    if ts.run and L >= 100:
        run = ts.run                                   # T*16: the free-slot mark; t_off8's A*16: k0 = 0, the smallest key
        # a window equal to the set's own smallest key (what k_dm_fill_finish fills the free slots with), without a pattern
        k0 = min((k for k in anchor_key_strings(c.patterns, ts.low) if k != b"T" * 16), key=lambda k: key_value(k))
        for o in (0, 8, 16, 5, L - 16):
            c.add("bare_k0", rs._place(rng, L, o, k0), False)
        for bare in (b"T" * 16, b"A" * 16):
            for o in (0, 8, 16, 64, 5, 13, L - 16, L - 19):
                s = bytearray(rs._place(rng, L, o, bare))
                if o:
                    s[o - 1] = ord("C")
                if o + 16 < L:
                    s[o + 16] = ord("C")
                c.add("bare_run_%s" % bare[:1].decode(), bytes(s), False)
        for tag, p in list(full.items()) + list(plain.items()):
            at = p.find(run)
            if at < 0:
                continue
            for o in (0, 3, 8, 11):                    # the pattern around the run, the run 8-aligned or not
                c.add("run_in_pattern", rs._place(rng, L, o, p), True)
                for d in (0, 7, 15):
                    q = bytearray(p)
                    q[at + d] = ord("G")
                    c.add("run_one_base_changed", rs._place(rng, L, o, bytes(q)), False)


_CASES = {}


def case(name, layout="u150"):
    """the designed reads of a named token set on a named layout (LAYOUTS), built once: a recruit_sets.Case whose patterns are the
    reference's"""
    key = (name, layout)
    if key in _CASES:
        return _CASES[key]
    ts = token_set(name)
    rng = random.Random("merge reads %s %s" % key)
    c = rs.Case(ts.reference[1])
    if layout == "ragged":
        for L in (60, 129, 300, 333):
            _design(c, ts, L, rng)
        rs.finish(c, max(N_READS[layout], len(c.seqs) + 300), lambda r: r.choice((40, 100, 150, 333, 700, r.randint(30, 700))), rng)
    else:
        L = int(layout[1:])
        _design(c, ts, L, rng)
        rs.finish(c, max(N_READS[layout], len(c.seqs) + 300), lambda r: L, rng)
    if len(c.seqs) % 64 == 0:
        c.add("background", _rand(rng, len(c.seqs[-1])), False)
    _CASES[key] = c
    return c
