"""Designed reads at the library's length limit (28 001 .. 60 000 bases): every array, every single repeat copy and every
background read is placed by hand, seeded, so that the oracle's answer can be written down from the design alone
(test_long_limit_sets_host.py pins it) and the GPU tests (test_gpu_long_reads_limit.py) cannot pass on an empty answer.

An array is DR, spacer, DR, ..., DR.  The bases next to a repeat cycle through ACGT from repeat to repeat, so that no column
beside the repeats reaches extendPreRepeat's vote (libcrispr.cpp:520-772) and the start/stops are the placed ones; spacers are
random, 30..40 bases, their first and last base being those flanks."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
RC = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
MAX_READ_LEN = 60000                    # CRASS_HIP_MAX_READ_LEN
LDS_BYTES = 160 * 1024


def revcomp(s):
    return s.translate(RC)[::-1]


def full_layout_bytes(L, window=8, low_sp=26, row_len=None):
    """survivor_lds_layout's total for a set whose longest read has L bases (survivor_wave.hip): ASCII copy, start/stop list and sims,
    two rows of 16-bit cells, packed words, hint words.  row_len: the longest string the rows hold (None: the read itself)."""
    seq = (L + 32 + 15) & ~15
    ss_cap = (2 * (L // (window + low_sp) + 4) + 3) & ~3
    row = (min(L, L if row_len is None else row_len) + 8 + 7) & ~7
    words = ((L + 15) // 16 + 2 + 3) & ~3
    hints = (((L + 63) // 64 + 2 + 1) & ~1) + 4
    return seq + ss_cap * 4 + 2 * row * 2 + words * 4 + ss_cap * 4 + hints * 8


def last_full_rows_length(**kw):
    """the longest read for which rows of the read's own length still fit a CU's LDS, under the given options"""
    L = max(l for l in range(1000, MAX_READ_LEN + 1) if full_layout_bytes(l, **kw) <= LDS_BYTES)
    assert full_layout_bytes(L + 1, **kw) > LDS_BYTES
    return L


L_OK = last_full_rows_length()          # 27 9xx under the defaults: this length takes the old layout, the next one the bounded rows
ROWS_ALONE = 40953                      # 4 x (L + 8) bytes of rows pass 160 KB on their own from here on
assert 4 * ((ROWS_ALONE + 8 + 7) & ~7) > LDS_BYTES >= 4 * ((ROWS_ALONE - 1 + 8 + 7) & ~7)

# two direct repeats of 30 bases, not low-complexity, no 7-mer in common; DR_A is its own low-lexi form, DR_B's reverse
# complement is the smaller string (its reads are flipped: reverseStartStops)
DR_A = b"ACCGTTAGCATCGGATACGCTTAGGCATTC"
DR_B = b"TTGCGACCATAGGCTCAATCGGTACCGTAG"
assert DR_A < revcomp(DR_A) and revcomp(DR_B) < DR_B and len(DR_A) == len(DR_B) == 30


class Read:
    def __init__(self, name, seq, dr=None, starts=(), single=None, background=False):
        self.name, self.seq, self.dr, self.starts, self.single, self.background = name, seq, dr, list(starts), single, background

    @property
    def L(self):
        return len(self.seq)

    def want_ss(self):
        """pass 1's start/stops as the reference leaves them: as placed for a low-lexi DR, mirrored for a flipped read"""
        n = len(self.dr)
        ss = [x for s in self.starts for x in (s, s + n - 1)]
        if self.dr < revcomp(self.dr):
            return 1, ss
        return 0, [self.L - 1 - x for x in reversed(ss)]

    def want_single(self):
        """pass 2's record of the one copy: (low_lexi, [start, end]) by the same rule"""
        dr, at = self.single
        if dr < revcomp(dr):
            return 1, [at, at + len(dr) - 1]
        return 0, [self.L - at - len(dr), self.L - 1 - at]


def _random(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].copy()


def _place_array(rng, s, dr, first, n_rep, end_at=None):
    """n_rep copies of dr from `first` on (or so that the last copy ends at end_at); returns the starts"""
    d = np.frombuffer(dr, np.uint8)
    gaps = [int(rng.integers(30, 41)) for _ in range(n_rep - 1)]
    if end_at is not None:
        first = end_at - (n_rep * len(d) + sum(gaps))
    starts, pos = [], first
    for k in range(n_rep):
        s[pos:pos + len(d)] = d
        starts.append(pos)
        if pos > 0:
            s[pos - 1] = ACGT[k % 4]                     # left flank of repeat k
        if pos + len(d) < len(s):
            s[pos + len(d)] = ACGT[(k + 1) % 4]          # right flank of repeat k
        if k < n_rep - 1:
            pos += len(d) + gaps[k]
    assert starts[-1] + len(d) <= len(s)
    # no spacer holds a 7-mer of the repeat by chance (scanRight takes the leftmost copy of the seed window in its range,
    # libcrispr.cpp:170-263: a chance copy inside a spacer would end the chain there)
    kmers = {dr[i:i + 7] for i in range(len(dr) - 6)}
    for k in range(n_rep - 1):
        a, b = starts[k] + len(d) + 1, starts[k + 1] - 1        # the spacer's inside, flanks kept
        while any(s[i:i + 7].tobytes() in kmers for i in range(a - 6, b)):       # every window that overlaps the inside
            s[a:b] = _random(rng, b - a)
    return starts


def build(seed=20261019):
    """the set: a list of Read, long reads spread over both halves (a group of two contexts holds some in each shard)"""
    rng = np.random.default_rng(seed)
    reads = []

    def bg(name, L):
        reads.append(Read(name, _random(rng, L).tobytes(), background=True))

    def arr(name, L, dr, n_rep, first=None, end_at=None, edit=None):
        s = _random(rng, L)
        starts = _place_array(rng, s, dr, first, n_rep, end_at)
        if edit:
            pos, ch = edit(starts)
            assert not any(st - 1 <= pos <= st + len(dr) for st in starts)      # inside a spacer, off the flanks
            s[pos] = ord(ch)
        reads.append(Read(name, s.tobytes(), dr=dr, starts=starts))

    def single(name, L, dr, at):
        s = _random(rng, L)
        s[at:at + len(dr)] = np.frombuffer(dr, np.uint8)
        reads.append(Read(name, s.tobytes(), single=(dr, at)))

    bg("bg150a", 150)
    arr("small3000", 3000, DR_A, 4, first=1200)
    bg("noarray10k", 10000)                                         # the light walk alone decides it
    bg("noarray_L_OK", L_OK)                                        # handed over by the light walk: longer than 12 288 bases
    arr("tail_L_OK+1", L_OK + 1, DR_A, 3, end_at=L_OK + 1 - 7)      # three repeats in the last 200 bases: searchEnd
    arr("straddle32768", ROWS_ALONE - 1, DR_B, 6, first=32768 - 170)
    single("single_at0", 3000, DR_A, 0)
    single("single_beyond32768", ROWS_ALONE, DR_A, 36000)
    arr("many130", MAX_READ_LEN - 1, DR_B, 130, first=20011)        # 260 start/stops: beyond the capped list of 256
    bg("bg150b", 150)
    arr("wide_beyond41000", MAX_READ_LEN, DR_A, 90, first=41077)    # ~5.8 kbp: beyond the 4 608-byte ASCII window
    arr("tail_at_L", MAX_READ_LEN, DR_A, 3, end_at=MAX_READ_LEN)    # the last repeat ends with the read
    single("single_ends_at_L", MAX_READ_LEN - 1, DR_A, MAX_READ_LEN - 1 - 30)
    single("single_in_60000", MAX_READ_LEN, DR_B, 47001)            # a 60 000-base read pass 1 does not find
    arr("straddle32768_N", 45000, DR_A, 5, first=32768 - 100, edit=lambda st: (st[1] + 45, "N"))        # k_survivor<true>
    arr("tail_lowercase", 52000, DR_B, 3, end_at=52000 - 40, edit=lambda st: (st[0] + 47, "g"))         # k_survivor<true>
    bg("bg3000", 3000)
    bg("noarray45k", 45001)
    assert [r.L for r in reads].count(MAX_READ_LEN) >= 3 and max(r.L for r in reads) == MAX_READ_LEN
    return reads


_cache = {}


def get(seed=20261019):
    if seed not in _cache:
        _cache[seed] = build(seed)
    return _cache[seed]


def subset_up_to(reads, max_len):
    """the reads of at most max_len bases: a set whose longest read has exactly that length when one of them has"""
    return [r for r in reads if r.L <= max_len]
