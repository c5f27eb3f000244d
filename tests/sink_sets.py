"""Designed dense read sets for the ORDERED SINKS of both passes (CPU only, seeded, deterministic): the compactions and gathers of
sinks.hip that turn "flag per slot" into "records in ascending read order, tokens in first-occurrence order, nothing dropped or
doubled".  Every layout puts a record on BOTH sides of a tile, block or word boundary of one of these kernels, and every layout's
expected answer is the whole of orc.pipeline on the same reads (test_sink_sets_host.py pins the designs on the CPU,
test_gpu_sinks.py runs them on the GPU).

THE CONSTANTS THE POSITIONS REST ON (read from the code, restated here so that a change there is seen here)

  lookback_tile_words(n_words)   engine_internal.h: 256 mask words per tile below 16 384 words, 4 096 from 16 384 words on
                                 (k_mask_compact_lb<256, 1> / <1024, 4>).  One word is 64 reads: tiles of 16 384 reads up to
                                 1 048 512 reads, of 262 144 reads from 1 048 513 reads on.  The three-kernel form
                                 (k_mask_count -> k_block_scan -> k_mask_scatter, CRASS_NO_LOOKBACK=1 and the long-read host loop)
                                 works in blocks of 256 words at every size.
  kFcTile = 16 384               sinks.hip, k_found_compact: 1 024 threads x 16 survivor slots; wave w of the block takes slots
                                 [1 024 w, 1 024 (w + 1)) of the tile in 16 steps of 64.  Launched for the survivor BOUND; tiles past
                                 the device-side count leave without drawing a ticket.
  GF_BLOCK = 1 024, GF_SLOTS = 2 048   k_gather_found: a block of 1 024 found records claims its strings in an LDS table of 2 048
                                 slots (at most 1 024 distinct keys), one thread per distinct string of the block then goes to the
                                 global de-duplication table.  Its `look` branch (read a slot before the CAS / atomicMin) is taken
                                 when the launch bound n_max exceeds 2^20 records; n_max is the survivor bound of the call.
  1 024                          k_dx_flag_compact: one candidate per thread, tiles of 1 024 candidates (found records in read
                                 order); candidate k is a first occurrence iff first[slot_of[k]] == k.
  kLbElemsPerTile = 4 096        k_valid_compact (lb_rank4): 1 024 threads x 4 consecutive hit slots.
  survivor_bound(n)              engine_ctx.h: min(max(65 536, (n + n / 2 + 65 535) & ~65 535), 2^26): what the NEXT call of a
                                 context sizes its survivor stage with.  It first exceeds 2^20 at n = 699 052 (n + n / 2 must
                                 reach 1 048 577; at 699 051 it is 1 048 576 and the bound is exactly 2^20).  hit_bound(n) =
                                 max(4 096, (n + n / 2 + 4 095) & ~4 095) is its pass-2 counterpart.
  Look-back bookkeeping          engine_ctx.h, next_lookback_tiles: one status array and one self-resetting ticket per context, a
                                 30-bit epoch per launch; the status array is grown to 2 x the tiles asked for (at least 4 096
                                 words) and zeroed only when it grows.

A READ FOUND IN PASS 1 TAKES NO HIT SLOT IN PASS 2.  pass2.hip: every probe and every recruit kernel tests
found_flag[rd_header_id(R, r)] before it looks at a read (anchor_filter_body, k_recruit, k_recruit_wide), so a found read never
sets its bit of the hit mask.  The hit slots are the FLAGGED reads in ascending read order (the read-mask compaction), here the
R and V reads; the F reads in front of a P layout shift read indices, not slot ranks.

RANKS.  Survivor slot s is rank s in the survivor list (F and S reads in ascending read order); k_found_compact gives fidx[k] = s
for the k-th found slot and k_gather_found labels record k with surv_idx[fidx[k]].  Candidate k is the k-th found record.  Hit
slot k is rank k among the flagged reads, vidx[q] the slot of the q-th valid one.

THE CLASSES (default options, reads of 80 bases unless a layout says otherwise; classified by the reference side only)
  F  found: two copies of a 23 .. 27 base repeat around a 26 .. 29 base spacer; kept when orc.pipeline([s]).n_pass1 == 1 and
     edge_reads.lattice_hit(s).  Pass 1 looks at one read at a time, so an F read is found in every set.
  S  survives the filter, not found: a random read with the 8-mer of a lattice seed copied 49 bases on; kept when lattice_hit is
     true and the oracle finds nothing.  Every filter is a superset of the lattice test: S reads are survivors on every route.
  Z  nothing: random, edge_reads.padded_model false.  Every filter's documented superset lies inside that model.
  R  recruited: a Z background with one copy of a PATTERN of the layout (orc.pipeline over the layout's F reads; pass 1 and the
     merge see only those, so the pattern set of the final set is the same), padded_model false.  Which strings stay patterns
     is the merge's decision, hence R is confirmed per layout from the oracle's result on the final set.
  V  flagged by pass 2's probe, rejected by the verify: a pattern with its LAST base changed, placed at a read offset that is
     a multiple of 8, so that the key P[0:16] sits in an aligned window (build_anchors); kept when padded_model is false and no
     pattern of the layout occurs in the read.  THAT THE PROBE FLAGS THE READ IS BY CONSTRUCTION AND CANNOT BE OBSERVED: the
     library reports no per-read flag, and a V read that went unflagged would give the same records.  (n_bound_overflows[2] and
     the learnt hit bound are the only trace.)
  A/B  an F template A and its reverse complement B: the same low-lexi string, hence one token, with opposite rec_lowlexi.

Reads may repeat: the Z, S, R and V reads of a layout are drawn (seeded) from small pools, the F reads from templates.  The sinks
see slots, not bases; neighbours differ, so a record shifted by one slot differs in its fields as well as in rec_read.

LAYOUTS (names of LAYOUTS; each a function of no arguments returning a Layout, cached)
  M1-n   read-mask tiles, n in 16 383, 16 384, 16 385, 32 769: Z everywhere; F at reads 0, 63, 64, 16 383, 16 384, 32 767,
         32 768 and n - 1 where they exist, an S beside each, an R two away.  n mod 64 != 0 covers a partial last mask word.
  M2-n   the fat-tile switch, n in 1 048 512 (64 tiles of 256 words), 1 048 513 (4 tiles of 4 096 words), 1 048 577 (5, the
         last of one word): the same around reads 262 143 / 262 144, 524 287 / 524 288, 1 048 511 / 1 048 512 and
         1 048 575 / 1 048 576.
  F1-n-pattern   every read F or S (slot = read index), n in 16 383, 16 384, 16 385, 49 153; patterns allF, edges (all S but F at
         the edges of 16 384, and of its multiples at 49 153), alt (F at even slots), mid (49 153: the whole middle tile S), allS
         (nothing found: an empty merge, pass 2 without a pattern).  F1-16385-altZ: every survivor of alt followed by a Z read.
  D1     66 561 F reads (65 tiles of 1 024 candidates + 1), all of repeat #0 but the first occurrences of repeats #1 .. #9 at
         candidate ranks 1, 1 023, 1 024, 1 025, 2 047, 2 048, 65 535, 65 536, 66 560; #1 is A and #4 (rank 1 025) is B.
  D2     2 049 F reads: ranks 0 .. 1 023 carry 1 024 distinct repeats (the limit of the gather block's LDS table), ranks
         1 024 .. 2 047 the same in reverse order, the last read a new one.
  D3     699 052 F reads cycling over 40 templates: survivor_bound(n) > 2^20, so the second and later steps of a context run
         k_gather_found with `look`.
  P1-h-pattern   8 F reads for the patterns, then h reads of R or V (hit slot k = read 8 + k), h in 4 095, 4 096, 4 097, 12 289;
         patterns allR, edges, alt, mid (12 289), allV (zero recruits).
  P2     8 F reads + 266 241 R reads: 65 tiles of 4 096 hit slots + 1.
  W-L    about 200 reads of L in 255, 256, 257 bases: F reads whose last repeat ends on the read's last base and F reads whose
         array starts at base 0, R reads whose copy ends on the last base (the largest start) and at base 0, Z reads.  Pass 1
         stores start/stops as bytes up to 256 bases and as 16 bits beyond; pass 2's 9-byte record serves up to 255 bases.
  H-edges, H-alt   16 385 reads of 2 049 bases (the long-read host loop: three-kernel compaction, k_gather_sparse): arrays in
         reads 0, 63, 64, 16 383, 16 384, or in every other read.  Backgrounds are plain random; whatever else they yield is
         the oracle's answer.

"Edges of T": ranks 0, 1, 63, 64, T - 1, T, T + 1 and the last one, plus 1 023 and 1 024 where T > 1 024.
Layout.bounds lists (space, rank below, rank on) for every boundary that has a record on both sides by design; spaces: "read"
(read index, F there), "surv" (survivor rank, found), "cand" (candidate rank, a first occurrence), "hit" (hit slot, recruited).
"""
import functools
from collections import namedtuple

import numpy as np

from tests import orc
from tests import edge_reads as E

P = orc.Params.default()
L0 = 80
T_MASK_SMALL, T_MASK_FAT, FAT_FROM_WORDS = 256, 4096, 16384      # lookback_tile_words
T_FOUND = 16384                                                   # kFcTile
T_GATHER = 1024                                                   # GF_BLOCK
T_CAND = 1024                                                     # k_dx_flag_compact
T_HIT = 4096                                                      # kLbElemsPerTile
N_P_FRONT = 8                                                     # F reads in front of a P layout
D1_RANKS = (1, 1023, 1024, 1025, 2047, 2048, 65535, 65536, 66560)
D1_A, D1_B = 1, 4                                                 # repeats #1 and #4 of D1 are A and B

_RC = bytes.maketrans(b"ACGT", b"TGCA")

Tmpl = namedtuple("Tmpl", "seq token low")


def revcomp(s):
    return s.translate(_RC)[::-1]


def lookback_tile_words(n_words):
    return T_MASK_FAT if n_words >= FAT_FROM_WORDS else T_MASK_SMALL


def survivor_bound(n):
    return min(max(65536, (n + n // 2 + 65535) & ~65535), 1 << 26)


def hit_bound(n):
    return max(4096, (n + n // 2 + 4095) & ~4095)


def first_n_with_look():
    """the smallest n whose survivor bound exceeds 2^20 (the bound is monotone: bisection)"""
    lo, hi = 1, 1 << 21
    while lo < hi:
        mid = (lo + hi) // 2
        if survivor_bound(mid) > (1 << 20):
            hi = mid
        else:
            lo = mid + 1
    return lo


def edges(T, last):
    r = {0, 1, 63, 64, T - 1, T, T + 1, last}
    if T > 1024:
        r |= {1023, 1024}
    return sorted(x for x in r if 0 <= x <= last)


class Layout:
    """buf / off: the reads; F, S, Z, R, V: ascending read indices by class; bounds: see the module docstring; tokens: the designed
    first-occurrence order (D1, D2) or None; ab: read indices of an A read and a B read, or None"""

    def __init__(self, name, rows, kinds, bounds=(), tokens=None, ab=None, exact=True):
        self.name, self.n, self.L = name, rows.shape[0], rows.shape[1]
        self.buf = np.ascontiguousarray(rows).reshape(-1)
        self.off = np.arange(self.n + 1, dtype=np.uint64) * np.uint64(self.L)
        self.kinds = kinds
        for k in "FSZRV":
            setattr(self, k, np.flatnonzero(kinds == ord(k)))
        self.bounds, self.tokens, self.ab, self.exact = list(bounds), tokens, ab, exact

    @property
    def reads(self):
        return self.buf, self.off

    def rows(self):
        return self.buf.reshape(self.n, self.L)

    def read(self, i):
        return self.buf[i * self.L:(i + 1) * self.L].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# templates and pools
# ---------------------------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return E.LETTERS[rng.integers(0, 4, n)]


def _is_f(s):
    r = orc.pipeline([s])
    if r.n_pass1 == 1 and E.lattice_hit(s, P):
        return Tmpl(s, bytes(r.tokens[0]), int(r.rec_lowlexi[0]))
    return None


@functools.lru_cache(maxsize=None)
def f_templates(n, L=L0, seed=11):
    """n F templates with pairwise distinct tokens, and the A/B pair: ([Tmpl] with A at index 1, B)"""
    rng = np.random.default_rng([seed, L, 1])
    out, seen, b = [], set(), None
    while len(out) < n or b is None:
        r, s = int(rng.integers(23, 28)), int(rng.integers(26, 30))
        if 2 * r + s > L - 1:
            continue
        a = _rand(rng, L)
        at = int(rng.integers(0, L - 1 - (2 * r + s) + 1))
        a[at + r + s:at + 2 * r + s] = a[at:at + r]
        t = _is_f(a.tobytes())
        if t is None or t.token in seen:
            continue
        if b is None and len(out) == 1:                        # is this one an A?
            tb = _is_f(revcomp(t.seq))
            if tb is None or tb.token != t.token or tb.low == t.low:
                continue
            b = tb
        seen.add(t.token)
        out.append(t)
    return out[:n], b


@functools.lru_cache(maxsize=None)
def s_pool(n=256, L=L0, seed=12):
    rng = np.random.default_rng([seed, L])
    sh = E.shape(P, L)
    out = []
    while len(out) < n:
        a = _rand(rng, L)
        j = sh.skips * int(rng.integers(0, sh.searchEnd // sh.skips + 1))
        a[j + sh.D0:j + sh.D0 + sh.w] = a[j:j + sh.w]
        s = a.tobytes()
        if E.lattice_hit(s, P) and orc.pipeline([s]).n_pass1 == 0:
            out.append(a)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def z_pool(n=4096, L=L0, seed=13):
    return E.backgrounds(np.random.default_rng([seed, L]), P, L, n)[0]


def patterns_of(f_rows):
    """the pattern set pass 2 gets when these are the set's found reads"""
    n, L = f_rows.shape
    r = orc.pipeline((np.ascontiguousarray(f_rows).reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(L)), do_pass2=False)
    return [bytes(p) for p in r.patterns]


def planted(rng, L, pats, n, where="any", spoil=False):
    """n Z backgrounds with one pattern each (cycling over pats) — R reads; spoil: its last base changed, at a multiple of 8,
    and no pattern in the read — V reads"""
    out, k = [], 0
    assert pats
    while len(out) < n:
        bg = E.backgrounds(rng, P, L, max(64, min(2048, n - len(out))))[0].copy()
        for a in bg:
            m = np.frombuffer(pats[k % len(pats)], np.uint8).copy()
            k += 1
            room = L - len(m)
            if spoil:
                m[-1] = E.LETTERS[(E._CODE[m[-1]] + int(rng.integers(1, 4))) & 3]
                at = 8 * int(rng.integers(0, room // 8 + 1))
            else:
                at = {"any": int(rng.integers(0, room + 1)), "end": room, "start": 0}[where]
            a[at:at + len(m)] = m
        ok = ~E.padded_model_batch(bg, P)
        for a in bg[ok]:
            if spoil:
                s = a.tobytes()
                if any(p in s for p in pats):
                    continue
            out.append(a)
    return np.stack(out[:n])


def _assemble(name, L, kinds, f_rows, rng, seed_bounds=(), r_where="any", **kw):
    """kinds: uint8 array of F / S / Z / R / V per read; f_rows: the F reads' rows in read order"""
    n = len(kinds)
    rows = np.empty((n, L), np.uint8)
    fi = np.flatnonzero(kinds == ord("F"))
    assert len(fi) == len(f_rows)
    if len(fi):
        rows[fi] = f_rows
    for k, pool in (("S", s_pool), ("Z", z_pool)):
        idx = np.flatnonzero(kinds == ord(k))
        if len(idx):
            p = pool(L=L)
            rows[idx] = p[rng.integers(0, len(p), len(idx))]
    ri, vi = np.flatnonzero(kinds == ord("R")), np.flatnonzero(kinds == ord("V"))
    if len(ri) or len(vi):
        pats = patterns_of(rows[fi])
        if len(ri):
            p = planted(rng, L, pats, min(len(ri), 2048), r_where)
            rows[ri] = p[rng.permutation(len(ri)) % len(p)]
        if len(vi):
            p = planted(rng, L, pats, min(len(vi), 512), spoil=True)
            rows[vi] = p[rng.permutation(len(vi)) % len(p)]
    return Layout(name, rows, kinds, seed_bounds, **kw)


def _f_rows(tm, sel):
    t = np.stack([np.frombuffer(x.seq, np.uint8) for x in tm])
    return t[np.asarray(sel, np.int64)]


def _rng(*key):
    return np.random.default_rng([77] + [int(k) for k in key])


# ---------------------------------------------------------------------------------------------------------------------------------
# the layouts
# ---------------------------------------------------------------------------------------------------------------------------------
def _mask_layout(name, n, f_at, pairs, key):
    rng = _rng(*key)
    kinds = np.full(n, ord("Z"), np.uint8)
    f_at = sorted({x for x in f_at if 0 <= x < n})
    kinds[f_at] = ord("F")
    for k, d in (("S", 1), ("R", 2)):
        for f in f_at:
            for q in (f + d, f - d, f + d + 2, f - d - 2, f + d + 4, f - d - 4):
                if 0 <= q < n and kinds[q] == ord("Z"):
                    kinds[q] = ord(k)
                    break
            else:
                raise AssertionError("no room beside %d" % f)
    tm = f_templates(40)[0]
    bounds = [("read", a, b) for a, b in pairs if b < n]
    return _assemble(name, L0, kinds, _f_rows(tm, np.arange(len(f_at)) % len(tm)), rng, bounds)


def m1(n):
    return _mask_layout("M1-%d" % n, n, [0, 63, 64, 16383, 16384, 32767, 32768, n - 1], [(63, 64), (16383, 16384), (32767, 32768)], (1, n))


def m2(n):
    return _mask_layout("M2-%d" % n, n, [0, 63, 64, 262143, 262144, 524287, 524288, 1048511, 1048512, 1048575, 1048576, n - 1],
                        [(63, 64), (262143, 262144), (524287, 524288), (1048511, 1048512), (1048575, 1048576)], (2, n))


def _tile_pattern(n, T, pattern, yes, no):
    """the F1 / P1 patterns over n slots with tiles of T"""
    kinds = np.full(n, ord(no), np.uint8)
    bounds = []
    mult = [k * T for k in range(1, (n - 1) // T + 1)]
    if pattern in ("all" + yes, "edges"):
        if pattern == "edges":
            at = set(edges(T, n - 1))
            for b in mult:
                at |= {b - 1, b, b + 1}
            kinds[sorted(x for x in at if x < n)] = ord(yes)
        else:
            kinds[:] = ord(yes)
        bounds = [(63, 64), (1023, 1024)] + [(b - 1, b) for b in mult]
    elif pattern == "alt":
        kinds[0::2] = ord(yes)
    elif pattern == "mid":
        assert n > 2 * T
        kinds[:] = ord(yes)
        kinds[T:2 * T] = ord(no)
        bounds = [(63, 64), (1023, 1024)] + [(b - 1, b) for b in mult if b > 2 * T]
    else:
        assert pattern == "all" + no, pattern
    return kinds, bounds


def f1(n, pattern):
    rng = _rng(3, n, sum(pattern.encode()))
    tm = f_templates(40)[0]
    if pattern == "altZ":
        k0, _ = _tile_pattern(n, T_FOUND, "alt", "F", "S")
        kinds = np.full(2 * n, ord("Z"), np.uint8)
        kinds[0::2] = k0
        bounds = []
    else:
        kinds, b = _tile_pattern(n, T_FOUND, pattern, "F", "S")
        bounds = [("surv", x, y) for x, y in b]
    nf = int((kinds == ord("F")).sum())
    return _assemble("F1-%d-%s" % (n, pattern), L0, kinds, _f_rows(tm, rng.integers(0, len(tm), nf)), rng, bounds)


def d1():
    n = 65 * T_CAND + 1
    tm, b = f_templates(1025)
    tm = list(tm[:10])
    tm[D1_B] = b
    sel = np.zeros(n, np.int64)
    for k, r in enumerate(D1_RANKS):
        sel[r] = k + 1
    tokens = [t.token for i, t in enumerate(tm) if i != D1_B]
    return _assemble("D1", L0, np.full(n, ord("F"), np.uint8), _f_rows(tm, sel), _rng(4),
                     [("cand", 1023, 1024), ("cand", 2047, 2048), ("cand", 65535, 65536)], tokens=tokens, ab=(D1_RANKS[D1_A - 1], D1_RANKS[D1_B - 1]))


def d2():
    tm = f_templates(1025)[0]
    sel = np.concatenate([np.arange(1024), np.arange(1023, -1, -1), [1024]])
    return _assemble("D2", L0, np.full(len(sel), ord("F"), np.uint8), _f_rows(tm, sel), _rng(5),
                     [("surv", 1023, 1024), ("surv", 2047, 2048)], tokens=[t.token for t in tm])


def d3():
    n = first_n_with_look()
    tm = f_templates(40)[0]
    return _assemble("D3", L0, np.full(n, ord("F"), np.uint8), _f_rows(tm, np.arange(n) % 40), _rng(6),
                     [("surv", 1023, 1024), ("surv", T_FOUND - 1, T_FOUND), ("surv", 42 * T_FOUND - 1, 42 * T_FOUND)])


def _p_layout(name, h, kinds_h, bounds, key):
    tm = f_templates(40)[0]
    kinds = np.concatenate([np.full(N_P_FRONT, ord("F"), np.uint8), kinds_h])
    return _assemble(name, L0, kinds, _f_rows(tm, np.arange(N_P_FRONT)), _rng(*key), [("hit", x, y) for x, y in bounds])


def p1(h, pattern):
    kinds, b = _tile_pattern(h, T_HIT, pattern, "R", "V")
    return _p_layout("P1-%d-%s" % (h, pattern), h, kinds, b, (7, h, sum(pattern.encode())))


def p2():
    h = 65 * T_HIT + 1
    return _p_layout("P2", h, np.full(h, ord("R"), np.uint8), [(k * T_HIT - 1, k * T_HIT) for k in range(1, 66)], (8,))


def _array_read(rng, L, at_end, bg):
    """a Z background of L bases with an array of 2 .. 4 repeats at its end (the last repeat ends on the last base) or at base 0"""
    r, nrep = int(rng.integers(23, 31)), int(rng.integers(2, 5))
    rep = _rand(rng, r)
    parts = [rep]
    for _ in range(nrep - 1):
        parts += [_rand(rng, int(rng.integers(26, 36))), rep]
    arr = np.concatenate(parts)
    a = bg.copy()
    if at_end:
        a[L - len(arr):] = arr
    else:
        a[:len(arr)] = arr
    return a


def w(L):
    rng = _rng(9, L)
    plan = np.array(list("FfRrZ" * 40))           # F: array at the end, f: at base 0, R: copy at the end, r: at base 0
    plan = plan[rng.permutation(len(plan))]
    n = len(plan)
    bgs = iter(E.backgrounds(rng, P, L, 4000)[0])
    f_rows = []
    for k in plan:
        if k in "Ff":
            while True:
                a = _array_read(rng, L, k == "F", next(bgs))
                s = a.tobytes()
                rc, ss, _ = orc.search_core(s, P)
                if rc == 1 and E.lattice_hit(s, P) and orc.pipeline([s]).n_pass1 == 1 and (k == "f" or max(ss) >= L - 1):
                    break
            f_rows.append(a)
    kinds = np.array([ord(k.upper()) for k in plan], np.uint8)
    lay = _assemble("W-%d" % L, L, kinds, np.stack(f_rows), rng)
    # R reads: the copy on the last base for "R", at base 0 for "r"
    pats = patterns_of(lay.rows()[lay.F])
    rows = lay.rows()
    for where, key in (("end", "R"), ("start", "r")):
        idx = np.flatnonzero(plan == key)
        rows[idx] = planted(rng, L, pats, len(idx), where)
    return Layout(lay.name, rows, kinds)


def h(which):
    n, L = 16385, 2049
    rng = _rng(10, sum(which.encode()))
    rows = E.LETTERS[rng.integers(0, 4, size=(n, L))]
    at = [0, 63, 64, 16383, 16384] if which == "edges" else list(range(0, n, 2))
    for i in at:
        while True:
            r = int(rng.integers(23, 33))
            rep = _rand(rng, r)
            arr = np.concatenate([rep, _rand(rng, int(rng.integers(28, 40))), rep, _rand(rng, int(rng.integers(28, 40))), rep])
            a = rows[i].copy()
            o = int(rng.integers(0, L - len(arr)))
            a[o:o + len(arr)] = arr
            if orc.search_core(a.tobytes(), P)[0] == 1:
                rows[i] = a
                break
    kinds = np.full(n, ord("Z"), np.uint8)          # (plain random backgrounds: "Z" here only means "not designed")
    kinds[at] = ord("F")
    return Layout("H-%s" % which, rows, kinds, [("read", 63, 64), ("read", 16383, 16384)] if which == "edges" else [], exact=False)


M1_N = (16383, 16384, 16385, 32769)
M2_N = (1048512, 1048513, 1048577)
F1_N = (16383, 16384, 16385, 49153)
P1_H = (4095, 4096, 4097, 12289)


def _registry():
    reg = {}
    for n in M1_N:
        reg["M1-%d" % n] = functools.partial(m1, n)
    for n in M2_N:
        reg["M2-%d" % n] = functools.partial(m2, n)
    for n in F1_N:
        for pat in ("allF", "edges", "alt", "allS") + (("mid",) if n == 49153 else ()):
            reg["F1-%d-%s" % (n, pat)] = functools.partial(f1, n, pat)
    reg["F1-16385-altZ"] = functools.partial(f1, 16385, "altZ")
    reg["D1"], reg["D2"], reg["D3"] = d1, d2, d3
    for hh in P1_H:
        for pat in ("allR", "edges", "alt", "allV") + (("mid",) if hh == 12289 else ()):
            reg["P1-%d-%s" % (hh, pat)] = functools.partial(p1, hh, pat)
    reg["P2"] = p2
    for L in (255, 256, 257):
        reg["W-%d" % L] = functools.partial(w, L)
    reg["H-edges"], reg["H-alt"] = functools.partial(h, "edges"), functools.partial(h, "alt")
    return reg


LAYOUTS = _registry()
BIG = {"M2-1048512", "M2-1048513", "M2-1048577", "D3"}       # built, used and dropped: never two of them in memory
_cache, _refs = {}, {}


def layout(name):
    if name not in _cache:
        if name in BIG:
            for k in list(_cache):
                if k in BIG:
                    del _cache[k]
                    _refs.pop(k, None)
        _cache[name] = LAYOUTS[name]()
    return _cache[name]


def reference(name):
    """the oracle's answer for the whole set, computed once and never changed"""
    if name not in _refs:
        lay = layout(name)
        _refs[name] = orc.pipeline(lay.reads)
    return _refs[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def ss_lists(res, lo, hi):
    """the start/stop lists of records lo .. hi - 1 concatenated in record order, through rec_ss_off"""
    nss = np.asarray(res.rec_nss[lo:hi], np.int64)
    off = np.asarray(res.rec_ss_off[lo:hi], np.int64)
    total = int(nss.sum())
    if total == 0:
        return np.zeros(0, np.uint32)
    start = np.cumsum(nss) - nss
    idx = np.repeat(off - start, nss) + np.arange(total, dtype=np.int64)
    return np.asarray(res.ss_pool, np.uint32)[idx]


def assert_same_arrays(gpu, ref):
    """what parity.assert_same_pipeline asserts (and pass 2's rec_replen as well), without a Python loop over the records: counts,
    every per-record field of both passes, the start/stop lists through rec_ss_off, tokens, groups, patterns and pat_group"""
    assert ref.error == 0
    assert (gpu.n_pass1, gpu.n_pass2) == (ref.n_pass1, ref.n_pass2), ((gpu.n_pass1, gpu.n_pass2), (ref.n_pass1, ref.n_pass2))
    n1, n = ref.n_pass1, ref.n_pass1 + ref.n_pass2
    for lo, hi, fields in ((0, n1, ("rec_read", "rec_lowlexi", "rec_replen", "rec_nss", "rec_token")),
                           (n1, n, ("rec_read", "rec_lowlexi", "rec_replen", "rec_nss", "rec_token"))):     # (pass 2: replen 0, nss 2 on both sides)
        for f in fields:
            np.testing.assert_array_equal(np.asarray(getattr(gpu, f))[lo:hi], np.asarray(getattr(ref, f))[lo:hi], err_msg=f)
        np.testing.assert_array_equal(ss_lists(gpu, lo, hi), ss_lists(ref, lo, hi), err_msg="start/stop lists")
    assert len(gpu.rec_read) == n
    assert (gpu.n_tokens, gpu.n_groups, gpu.n_patterns) == (ref.n_tokens, ref.n_groups, ref.n_patterns)
    assert [bytes(t) for t in gpu.tokens] == [bytes(t) for t in ref.tokens]
    assert [list(g) for g in gpu.groups] == [list(g) for g in ref.groups]
    assert [bytes(p) for p in gpu.patterns] == [bytes(p) for p in ref.patterns]
    np.testing.assert_array_equal(np.asarray(gpu.pat_group), np.asarray(ref.pat_group))
