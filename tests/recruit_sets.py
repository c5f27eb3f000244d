"""Pass 2 (findSingletons / on_match, libcrispr.cpp:399-518) on caller-given patterns: the plain reference, the pattern
sets that reach every route of crass_hip_set_patterns + crass_hip_recruit, and designed reads.  No GPU, no product code: the
first match comes from the oracle's byte-wise automaton (tests/orc.PatternSet), the reverse complement from its table.

A designed read is random filler with one copy (where a class says so, two) of a pattern of the set at a stated offset;
every designed read carries the verdict it was designed for (recruited or not), which test_recruit_sets_host.py checks
against the reference before any GPU test trusts either.  Everything is deterministic (fixed seeds)."""
import ctypes as C
import random

from tests import orc

# ---- thresholds of the product's routing, quoted where the tests assert them ----
LDS_256_MAX_STATES = 4096         # launch_recruit_lds: n_states * 10 bytes <= 40 KB -> 256 threads
LDS_512_MAX_STATES = 8192         # <= 80 KB -> 512 threads
LDS_1024_MAX_STATES = 16384       # <= 160 KB -> 1 024 threads; beyond: k_recruit<false> from global memory
GO4_MAX_STATES = 65535            # install_patterns: 16-bit tables up to here, go4w / go32 beyond
MODE0_MAX_KEYS = 16384            # build_anchors: exact keys in LDS, 2^15 slots at load <= 1/2
MODE1_MAX_KEYS = 52428            # fingerprint buckets, 2^16 slots at load <= 0.8; beyond: exact keys in L2 (log_size > 15)
ANCHOR_MIN_LEN = 23               # build_anchors gives up when an ACGT pattern is shorter


def revcomp(s):
    """reverseComplement by crass's table (orc_revcomp)"""
    out = C.create_string_buffer(len(s) + 1)
    orc.lib().orc_revcomp(bytes(s), len(s), out)
    return out.raw[:len(s)]


def record(r, seq, end_excl, length, less=lambda a, b: a < b, end_inclusive=False):
    """on_match + DRLowLexi for the single repeat of read r whose first callback is (end_excl, length)"""
    L = len(seq)
    dr_end = end_excl if end_inclusive else end_excl - 1
    if dr_end >= L:
        dr_end = L - 1
    start = dr_end - (length - 1)
    sub = bytes(seq[start:dr_end + 1])
    rc = revcomp(sub)
    if less(sub, rc):
        return (r, 1, start, dr_end, len(sub), sub)
    return (r, 0, L - 1 - dr_end, L - 1 - start, len(sub), rc)


def skipped_reads(n, found, header_id=None):
    """the reads findSingletons skips: those whose header id is the header id of a read listed in found"""
    hid = list(range(n)) if header_id is None else [int(h) for h in header_id]
    ids = {hid[int(f)] for f in found}
    return {r for r in range(n) if hid[r] in ids}


def find_singletons(seqs, patterns, found=(), header_id=None):
    """[(read, low_lexi, start, end, dr_len, dr_bytes)] in read order"""
    if not patterns:
        return []
    skip = skipped_reads(len(seqs), found, header_id)
    ps = orc.PatternSet(list(patterns), "oracle")
    out = []
    for r, s in enumerate(seqs):
        if r in skip:
            continue
        m = ps.first(s)
        if m:
            out.append(record(r, s, m[0], m[1]))
    ps.close()
    return out


def brute_first(seq, patterns, tie="longest"):
    """first callback by bytes.find over all patterns: the smallest end, among equal ends the longest pattern"""
    best = None
    for p in patterns:
        o = seq.find(p)
        if o < 0:
            continue
        key = (o + len(p), -len(p) if tie == "longest" else len(p))
        if best is None or key < best:
            best = key
    return None if best is None else (best[0], abs(best[1]))


class SliceMatcher:
    """the same first callback without walking the pattern list per read: the patterns by their last bases, one look-up per
    end position, the candidates compared longest first (for sets too large for bytes.find over every pattern)"""

    def __init__(self, patterns):
        self.k = min(12, min(len(p) for p in patterns))
        self.by_tail = {}
        for p in sorted(patterns, key=len, reverse=True):
            self.by_tail.setdefault(bytes(p[-self.k:]), []).append(bytes(p))

    def first(self, seq):
        k = self.k
        for e in range(k, len(seq) + 1):
            for p in self.by_tail.get(seq[e - k:e], ()):
                if len(p) <= e and seq[e - len(p):e] == p:
                    return (e, len(p))
        return None


def trie_states(patterns):
    """nodes of the patterns' trie, the root among them (= the automaton's states, counters' ac_states)"""
    seen = set()
    for p in patterns:
        for i in range(1, len(p) + 1):
            seen.add(p[:i])
    return len(seen) + 1


def anchor_keys(patterns):
    """distinct 16-mers p[r : r + 16], r = 0 .. 7, over the pure-ACGT patterns; None when one of them is shorter than 23"""
    keys = set()
    for p in patterns:
        if set(p) - set(b"ACGT"):
            continue
        if len(p) < ANCHOR_MIN_LEN:
            return None
        for r in range(8):
            keys.add(p[r:r + 16])
    return len(keys)


# ---- pattern sets ----
def _rand(rng, n):
    return bytes(rng.choices(b"ACGT", k=n))


def core_patterns(wide=False):
    """the patterns designed reads are made of, by name"""
    rng = random.Random(20240)
    c = {}
    for n in (23, 31, 32, 33, 47) + ((48, 63, 64, 65, 96) if wide else ()):
        c["p%d" % n] = _rand(rng, n)
    x = _rand(rng, 14)
    c["palin"] = x + revcomp(x)                        # equal to its own reverse complement
    c["long"] = _rand(rng, 40)
    c["suffix"] = c["long"][-25:]                      # proper suffix: same end, the longest wins
    c["outer"] = _rand(rng, 45)
    c["infix"] = c["outer"][5:28]                      # starts later, ends first
    assert c["palin"] == revcomp(c["palin"])
    return c


SHORT20 = _rand(random.Random(77), 20)
N_PATTERN = b"ACGGTCATTGCANGGTACCATGCAATTGC"
LOWER_PATTERN = b"TTGACCGATGCAtGGCATCGATCGGAT"


def pattern_set(name):
    """(patterns, core dict) of a named route (the table in test_gpu_recruit_routes.py)"""
    n_fill, lo, hi, extra, wide = {
        "lds256": (8, 23, 47, [SHORT20], False),
        "lds512": (160, 30, 40, [SHORT20], False),
        "lds1024": (330, 30, 40, [SHORT20], False),
        "general": (1000, 30, 40, [SHORT20], False),
        "go32": (2300, 30, 40, [SHORT20], False),
        "mode0": (1500, 23, 47, [], False),
        "mode0_small": (40, 23, 47, [], False),
        "mode0_wide": (300, 23, 96, [], True),
        "mode1": (2700, 23, 24, [], False),
        "mode2": (7000, 23, 24, [], False),
        "npat": (300, 23, 47, [N_PATTERN, LOWER_PATTERN], False),
    }[name]
    core = core_patterns(wide)
    rng = random.Random("patterns " + name)
    pats = list(core.values()) + list(extra)
    pats += [_rand(rng, rng.randint(lo, hi)) for _ in range(n_fill)]
    order = list(range(len(pats)))
    random.Random(5).shuffle(order)                    # the core is not the list's head
    pats = [pats[i] for i in order]
    assert len(set(pats)) == len(pats)
    if extra and extra[0] is SHORT20:
        core = dict(core, short=SHORT20)
    return pats, core


# ---- designed reads ----
class Case:
    """reads, patterns, and per class the designed reads [(read index, recruited?)]"""

    def __init__(self, patterns):
        self.patterns = patterns
        self.seqs = []
        self.classes = {}

    def add(self, cls, seq, recruited):
        self.classes.setdefault(cls, []).append((len(self.seqs), bool(recruited)))
        self.seqs.append(bytes(seq))

    @property
    def designed(self):
        return sorted(x for k, v in self.classes.items() if k != "background" for x in v)

    def want(self):
        return {i for i, rec in self.designed if rec}


def _place(rng, L, o, p):
    assert 0 <= o and o + len(p) <= L, (L, o, len(p))
    return _rand(rng, o) + p + _rand(rng, L - o - len(p))


def design(case, core, L, rng, exc=True, classes=None):
    """the designed reads of length L for the patterns in core (those that fit)"""
    def on(c):
        return classes is None or c in classes
    fit = {k: p for k, p in core.items() if len(p) <= L}
    singles = [k for k in fit if k not in ("suffix", "infix", "short")]
    for k in singles:
        p = fit[k]
        n = len(p)
        if on("window_start"):
            for o in range(0, 9):
                if o + n <= L:
                    case.add("window_start", _place(rng, L, o, p), True)
        if on("window_end"):
            for back in range(0, 9):
                if L - n - back >= 0:
                    case.add("window_end", _place(rng, L, L - n - back, p), True)
        if L > n and on("cut") and k not in ("long", "outer"):     # (their cut copies still hold "suffix" / "infix")
            case.add("cut_end", _rand(rng, L - n + 1) + p[:-1], False)
            case.add("cut_start", p[1:] + _rand(rng, L - n + 1), False)
        if on("near_miss"):
            for o in (0, 1, 7, 8, 9):
                if o + n <= L and k not in ("long", "outer"):
                    q = bytearray(p)
                    q[20] = ord("ACGT"[(b"ACGT".index(q[20]) + 1 + o % 3) % 4])
                    case.add("near_miss", _place(rng, L, o, bytes(q)), False)
        if on("start16"):
            for o in (16, 32, 48):
                if o + n <= L:
                    case.add("start16", _place(rng, L, o, p), True)
    if on("first_callback"):
        if "outer" in fit:
            for o in (0, 3, L - 45):
                case.add("first_callback_infix", _place(rng, L, o, fit["outer"]), True)
        if "long" in fit:
            for o in (0, 5, L - 40):
                case.add("first_callback_suffix", _place(rng, L, o, fit["long"]), True)
        tw = fit.get("short", fit.get("p23"))
        if tw and 2 * len(tw) + 9 <= L:
            for o in (0, 4):
                s = bytearray(_rand(rng, L))
                s[o:o + len(tw)] = tw
                s[L - len(tw):] = tw
                case.add("first_callback_twice", s, True)
    if on("palindrome") and "palin" in fit:
        for o in (0, 1, L - 28):
            case.add("palindrome", _place(rng, L, o, fit["palin"]), True)
    if exc and on("exception"):
        for k in ("p23", "p33", "p47"):
            if k not in fit or len(fit[k]) + 12 > L:
                continue
            p = fit[k]
            for o in (2, L - len(p) - 1):
                s = bytearray(_place(rng, L, o, p))
                s[0 if o else L - 1] = ord("N")                        # an N elsewhere
                case.add("exc_n_elsewhere", s, True)
                s = bytearray(_place(rng, L, o, p))
                s[o + len(p) // 2] = ord("N")                          # the copy interrupted
                case.add("exc_interrupted", s, False)
                s = bytearray(_place(rng, L, o, p))
                at = L - 1 if o < L - len(p) - 1 else 0
                s[at] = ord(chr(s[at]).lower())                        # a lower-case base elsewhere
                case.add("exc_lower_elsewhere", s, True)
        for p, cls in ((N_PATTERN, "exc_n_pattern"), (LOWER_PATTERN, "exc_lower_pattern")):
            if p in case.patterns and len(p) <= L:
                for o in (0, (L - len(p)) // 2, L - len(p)):
                    case.add(cls, _place(rng, L, o, p), True)


def design_slices(case, core, L, rng):
    """k_recruit_list_wave: 64 lanes, slices of seg = ceil(L / 64) bases; the copy of the longest pattern ends (last base) at
    the first base of a lane's slice, one before, one behind; two copies in different slices"""
    p = max(core.values(), key=len)
    n = len(p)
    seg = (L + 63) // 64
    for lane in (2, 17, 40, 63):
        s0 = lane * seg
        if s0 + 1 >= L or s0 - 1 - (n - 1) < 0:
            continue
        for d in (0, -1, 1):
            case.add("slice_edge", _place(rng, L, s0 + d - (n - 1), p), True)
    q = core["p23"]
    for a, b in ((5, 40), (20, 21), (1, 63)):
        s = bytearray(_rand(rng, L))
        oa, ob = a * seg + 3, min(b * seg + 1, L - n)
        s[oa:oa + len(q)] = q
        s[ob:ob + n] = p
        case.add("slice_two_copies", s, True)


def finish(case, n_total, lengths, rng):
    """random background reads (no pattern: the host test asserts it) up to n_total reads, designed reads spread among them"""
    designed = list(case.seqs)
    cls_of = {i: c for c, v in case.classes.items() for i, _ in v}
    rec_of = {i: r for v in case.classes.values() for i, r in v}
    n_bg = max(0, n_total - len(designed))
    total = len(designed) + n_bg
    slots = set((k * total) // len(designed) for k in range(len(designed))) if designed else set()
    assert len(slots) == len(designed)
    case.seqs, case.classes = [], {}
    d = 0
    for i in range(total):
        if i in slots:
            case.add(cls_of[d], designed[d], rec_of[d])
            d += 1
        else:
            case.add("background", _rand(rng, lengths(rng)), False)
    assert d == len(designed)
    return case


_CACHE = {}


def case(name, layout="u150", n_total=2003):
    """A named pattern set on a named read layout, built once.
    layouts: "uL" uniform reads of L bases; "padded": 140 .. 160 bases (one stride with pad_uniform=2); "ragged": 1 .. 700 bases
    (tight layout); "wL": uniform long reads (wave walk); "wragged": 2 100 .. 4 200 bases."""
    key = (name, layout, n_total)
    if key in _CACHE:
        return _CACHE[key]
    pats, core = pattern_set(name)
    rng = random.Random("reads %s %s" % (name, layout))
    c = Case(pats)
    if layout[0] == "u":
        L = int(layout[1:])
        design(c, core, L, rng)
        finish(c, n_total, lambda r: L, rng)
    elif layout == "padded":
        for L in (140, 141, 144, 147, 152, 153, 159, 160):
            design(c, core, L, rng, classes=("window_end", "cut", "near_miss", "exception", "palindrome"))
        finish(c, n_total, lambda r: r.randint(140, 160), rng)
    elif layout == "ragged":
        small = {k: core[k] for k in ("p23", "p32", "p33", "p47", "palin")}
        # a copy ending at the last base of a read of L % 16 in {1, 15, 0}; copies in the last window of a round of eight
        # windows (h % 8 == 7: offsets 49 .. 56 -> window 7) and the first of the next (57 .. 64 -> window 8)
        for k, p in small.items():
            for L in (len(p), 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113):
                if L >= len(p):
                    c.add("end_mod16", _place(rng, L, L - len(p), p), True)
            for o in list(range(49, 66)) + [120, 121, 127, 128, 129]:
                c.add("round_edge", _place(rng, o + len(p) + (o % 5), o, p), True)
        for L in (60, 129, 300, 699, 700):
            design(c, core, L, rng, classes=("window_start", "window_end", "cut", "near_miss", "first_callback", "exception"))
        for L in (1, 15, 16, 22, 23):
            for _ in range(3):
                c.add("short_read", _rand(rng, L), False)
        c.add("short_read_is_pattern", core["p23"], True)
        finish(c, n_total, lambda r: r.choice((1, 15, 16, 22, 23, 40, 100, 150, 333, 700, r.randint(1, 700))), rng)
    elif layout[0] == "w":
        wcore = {k: core[k] for k in ("p23", "p47", "palin", "long", "suffix", "outer", "infix")}
        def long_design(L):
            for k in ("p23", "p47"):
                p = wcore[k]
                for o in range(2033, 2049):            # window indices 255 and 256
                    if o + len(p) <= L:
                        c.add("window_255_256", _place(rng, L, o, p), True)
                    elif o + len(p) - 1 == L:
                        c.add("cut_end", _rand(rng, o) + p[:-1], False)
            design(c, wcore, L, rng, classes=("window_end", "cut", "near_miss", "first_callback", "palindrome", "exception"))
            design_slices(c, wcore, L, rng)
        if layout == "wragged":
            for L in (2100, 2577, 3072, 4200):
                long_design(L)
            finish(c, n_total, lambda r: r.randint(2100, 4200), rng)
        else:
            L = int(layout[1:])
            long_design(L)
            finish(c, n_total, lambda r: L, rng)
    else:
        raise KeyError(layout)
    _CACHE[key] = c
    return c


def head(c, n):
    """the first n reads of the sequence designed, background, designed, ... of a case, as a Case of its own"""
    d = [i for i, _ in c.designed]
    b = [i for i, _ in c.classes["background"]]
    order = [x for pair in zip(d, b) for x in pair][:n]
    cls_of = {i: k for k, v in c.classes.items() for i, _ in v}
    rec_of = {i: r for v in c.classes.values() for i, r in v}
    out = Case(c.patterns)
    for i in order:
        out.add(cls_of[i], c.seqs[i], rec_of[i])
    return out


# ---- the cases the GPU tests run, shared with the host test that pins them ----
# route -> (used_lds_automaton, anchor_table_kind or None, states (lo, hi], anchor keys (lo, hi] or None)
INF = 1 << 30
ROUTES = {
    "lds256": (1, None, (0, LDS_256_MAX_STATES), None),
    "lds512": (1, None, (LDS_256_MAX_STATES, LDS_512_MAX_STATES), None),
    "lds1024": (1, None, (LDS_512_MAX_STATES, LDS_1024_MAX_STATES), None),
    "general": (0, None, (LDS_1024_MAX_STATES, GO4_MAX_STATES), None),
    "go32": (0, None, (GO4_MAX_STATES, INF), None),
    "mode0": (2, 0, (0, GO4_MAX_STATES), (0, MODE0_MAX_KEYS)),
    "mode0_small": (2, 0, (0, GO4_MAX_STATES), (0, MODE0_MAX_KEYS)),
    "mode0_wide": (2, 0, (0, GO4_MAX_STATES), (0, MODE0_MAX_KEYS)),
    "mode1": (2, 1, (0, INF), (MODE0_MAX_KEYS, MODE1_MAX_KEYS)),
    "mode2": (2, 2, (GO4_MAX_STATES, INF), (MODE1_MAX_KEYS, INF)),
    "npat": (2, 0, (0, GO4_MAX_STATES), (0, MODE0_MAX_KEYS)),
}
ROUTE_CASES = [(r, "u150", 2003) for r in ("lds256", "lds512", "lds1024", "general", "go32", "mode0", "mode1", "mode2", "npat")]
UNIFORM_STRIDES = {49: 4, 64: 4, 65: 5, 80: 5, 128: 8, 192: 12, 193: 13, 208: 13, 241: 16, 256: 16, 257: 17}
WAVE_LENGTHS = (801, 2055, 2056, 2063, 2064, 2071)
LAYOUT_CASES = [("mode0", "u%d" % L, 2003) for L in UNIFORM_STRIDES] + [("mode0", "padded", 2003), ("mode0", "ragged", 2003)] + \
               [("mode0", "w%d" % L, 300) for L in WAVE_LENGTHS] + [("mode0", "wragged", 700), ("mode2", "w2064", 300)]
WIDE_CASES = [("mode0_wide", "u150", 2003), ("mode0_wide", "ragged", 2003)]           # highDRsize = 96
ALL_CASES = ROUTE_CASES + LAYOUT_CASES + WIDE_CASES + [("npat", "padded", 2003), ("mode0", "u150", 1025), ("mode0", "u150", 3073),
                                                        ("mode0_small", "u150", 2003)]
