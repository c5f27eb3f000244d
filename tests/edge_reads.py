"""Reads that sit on the edges of the pass-1 seed filter (CPU only, seeded, deterministic).

For a parameter set (orc.Params) and a read length L:
  w = searchWindowLength, skips = max(1, lowDR - (2w - 1)), searchEnd = L - lowDR - lowSp - w - 1,
  D0 = lowDR + lowSp, D1 = highDR + highSp.

* padded_model(read, params): some lattice seed j = i * skips <= searchEnd has its w-mer again at j + d, d in D0 .. D1, where
  bases at or past L and non-ACGT bytes read as 'A' (the packer's zero padding and its code for other bytes).  Every filter
  kernel's documented superset lies inside it (it ignores the reference's right clamp and the kernels' stride clamp), and so
  does the oracle's orc_has_lattice_hit.
* positive_set  (P): padded-model-free ACGT background + one exact copy of one lattice seed at an edge pair (j, d); every read
  is oracle-positive.
* negative_set  (N): the same background with near misses (one base of the copy changed, the copy at D0 - 1 or D1 + 1, an exact
  copy of the off-lattice seed j + 1); every read is padded-model-negative, hence oracle-negative.
* array_set     (A): real arrays whose first lattice hit is at an edge, and a few exception reads; all oracle-found.
* class_switch_set (S): a decoy copy that the oracle rejects, so that its seed loop leaves the lattice (libcrispr.cpp:390), and
  a real array behind it; kept only if the oracle finds the read after a class switch AND its record differs from the one for
  the same read without the decoy.
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from tests import orc

_CODE = np.zeros(256, np.uint8)
_CODE[ord("C")], _CODE[ord("G")], _CODE[ord("T")] = 1, 2, 3
LETTERS = np.frombuffer(b"ACGT", np.uint8)

Shape = namedtuple("Shape", "L w skips searchEnd D0 D1")


def params(**kw):
    return orc.Params.default(**kw)


def shape(p, L):
    w = int(p.searchWindowLength)
    skips = max(1, int(p.lowDRsize) - (2 * w - 1))
    return Shape(L, w, skips, L - int(p.lowDRsize) - int(p.lowSpacerSize) - w - 1, int(p.lowDRsize + p.lowSpacerSize),
                 int(p.highDRsize + p.highSpacerSize))


def has_seed(p, L):
    """(params, L) has at least one lattice seed with a distance that fits (else the sets are empty: skipped)"""
    s = shape(p, L)
    return s.searchEnd >= 0 and s.D1 >= s.D0


def padded_model_batch(a, p):
    """a: uint8 array (n, L) of ASCII reads of one length -> bool (n,): the padded superset model"""
    n, L = a.shape
    s = shape(p, L)
    if s.searchEnd < 0 or s.D1 < s.D0:
        return np.zeros(n, bool)
    span = s.searchEnd + s.D1 + 1                   # w-mers at positions 0 .. searchEnd + D1
    codes = np.zeros((n, span + s.w), np.uint32)     # (past L: 'A', the packer's zero padding)
    m = min(L, span + s.w)
    codes[:, :m] = _CODE[a[:, :m]]
    km = np.zeros((n, span), np.uint32)
    for i in range(s.w):
        km = (km << 2) | codes[:, i:i + span]
    seeds = np.arange(0, s.searchEnd + 1, s.skips)
    ks = km[:, seeds]
    hit = np.zeros(n, bool)
    for d in range(s.D0, s.D1 + 1):
        hit |= (ks == km[:, seeds + d]).any(axis=1)
    return hit


def padded_model(read, p):
    return bool(padded_model_batch(np.frombuffer(read, np.uint8).reshape(1, -1), p)[0])


def lattice_hit(read, p):
    """the oracle's test (orc_has_lattice_hit: searchCore's seed loop up to its first hit)"""
    return orc.lib().orc_has_lattice_hit(read, len(read), C.byref(p))


def class_switches(reset=False):
    r, c = C.c_uint64(), C.c_uint64()
    orc.lib().orc_stats_get(C.byref(r), C.byref(c), int(reset))
    return r.value, c.value


def backgrounds(rng, p, L, n):
    """n random ACGT reads of length L for which the padded model is false (rejection) -> (uint8 (n, L), rejection rate)"""
    out, tried = [], 0
    while sum(len(x) for x in out) < n:
        k = min(2000, max(64, 2 * (n - sum(len(x) for x in out))))
        a = LETTERS[rng.integers(0, 4, size=(k, L))]
        tried += k
        out.append(a[~padded_model_batch(a, p)])
    a = np.concatenate(out)[:n]
    return a, 1.0 - (sum(len(x) for x in out) / tried)


def edge_seeds(s):
    """lattice seeds at the filter's edges: 0, skips, the last one, word and halfword starts, the 32nd / 33rd seed (the 32-bit
    hint word), both sides of every 64-position hint tile boundary"""
    if s.searchEnd < 0:
        return []
    last = s.skips * (s.searchEnd // s.skips)
    js = {0, s.skips, last}
    lat = list(range(0, s.searchEnd + 1, s.skips))
    words = [j for j in lat if j % 16 in (0, 8)]
    js |= set(words[:3] + words[-3:])
    js |= {31 * s.skips, 32 * s.skips, 33 * s.skips}
    for t in range(64, s.searchEnd + 1, 64):
        js.add(s.skips * ((t - 1) // s.skips))
        js.add(s.skips * (-(-t // s.skips)))
    return sorted(j for j in js if 0 <= j <= s.searchEnd)


def dmax(s, j):
    """the reference's clamp: the copy of the seed at j must end before the read's last base (libcrispr.cpp:301-304)"""
    return min(s.D1, s.L - 1 - s.w - j)


def edge_distances(s, j):
    """D0, D0 + 1, dmax, dmax - 1, and distances that put the copy on / across a 16-base word boundary"""
    hi = dmax(s, j)
    ds = {s.D0, s.D0 + 1, hi, hi - 1}
    for r in {0, 8, 15, 16 - s.w // 2, 17 - s.w}:
        up = [d for d in range(s.D0, hi + 1) if (j + d) % 16 == r]
        if up:
            ds |= {up[0], up[-1]}
    return sorted(d for d in ds if s.D0 <= d <= hi)


def _plant(a, src, dst, w):
    a[dst:dst + w] = a[src:src + w]


@functools.lru_cache(maxsize=None)
def positive_set(pkey, L, reps=2, seed=1):
    """P: list[bytes].  pkey: a tuple of orc.Params fields (see key())"""
    p = orc.Params(*pkey)
    s = shape(p, L)
    if not has_seed(p, L):
        return []
    rng = np.random.default_rng([seed, L] + list(pkey))
    pairs = [(j, d) for j in edge_seeds(s) for d in edge_distances(s, j)]
    bg, _ = backgrounds(rng, p, L, len(pairs) * reps)
    out = []
    for i, (j, d) in enumerate(pairs * reps):
        a = bg[i].copy()
        _plant(a, j, j + d, s.w)
        r = a.tobytes()
        assert lattice_hit(r, p) == 1, (pkey, L, j, d)
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def negative_set(pkey, L, seed=2):
    """N: list[bytes]; near misses of the pairs of P"""
    p = orc.Params(*pkey)
    s = shape(p, L)
    if not has_seed(p, L):
        return []
    rng = np.random.default_rng([seed, L] + list(pkey))
    js = edge_seeds(s)
    plans = []
    # one base of the copy changed, at every window index, both bits of its code (xor 1, xor 2): every halfword and bit
    # position of the packed seed
    for j in sorted({js[0], js[-1]} | set(js[1:-1][::max(1, len(js) // 4)])):
        for d in sorted({s.D0, dmax(s, j)}):
            for t in range(s.w):
                for x in (1, 2):
                    plans.append(("mis", j, d, t, x))
    for j in js:
        plans.append(("copy", j, s.D0 - 1, 0, 0))                       # one short of D0
        if j + s.D1 + 1 + s.w <= L:
            plans.append(("copy", j, s.D1 + 1, 0, 0))                   # one beyond D1, where it fits
        if s.skips > 1:                                                 # the off-lattice seed j + 1, exact, at edge distances
            for d in edge_distances(s, j):
                if j + 1 + d + s.w <= L:
                    plans.append(("off", j, d, 0, 0))
    bg, _ = backgrounds(rng, p, L, len(plans))
    out = []
    for i, (kind, j, d, t, x) in enumerate(plans):
        a = bg[i].copy()
        if kind == "off":
            _plant(a, j + 1, j + 1 + d, s.w)
        else:
            _plant(a, j, j + d, s.w)
            if kind == "mis":
                a[j + d + t] = LETTERS[_CODE[a[j + d + t]] ^ x]
        if padded_model_batch(a.reshape(1, -1), p)[0]:
            continue                                                    # a chance hit: dropped
        r = a.tobytes()
        assert lattice_hit(r, p) == 0, (pkey, L, kind, j, d, t)
        out.append(r)
    return out


def key(p):
    return tuple(p.astuple())


def _rand(rng, n):
    return LETTERS[rng.integers(0, 4, n)]


def _mutate(rng, x, k):
    x = x.copy()
    for _ in range(k):
        i = int(rng.integers(0, len(x)))
        x[i] = LETTERS[_CODE[x[i]] ^ int(rng.integers(1, 4))]
    return x


def _array(rng, p, dr_len=None, sp_lens=None, n_rep=2, mut=0):
    """DR (spacer DR)*: uint8 array.  mut: up to that many point changes in every copy but the first"""
    lo, hi = int(p.lowDRsize), min(int(p.highDRsize), int(p.lowDRsize) + 12)
    dr = _rand(rng, dr_len or int(rng.integers(lo, hi + 1)))
    parts = [dr]
    for k in range(n_rep - 1):
        sl = sp_lens[k] if sp_lens else int(rng.integers(p.lowSpacerSize, min(p.highSpacerSize, p.lowSpacerSize + 8) + 1))
        parts += [_rand(rng, sl), _mutate(rng, dr, int(rng.integers(0, mut + 1))) if mut else dr]
    return np.concatenate(parts), len(dr)


@functools.lru_cache(maxsize=None)
def array_set(pkey, L, n_try=400, seed=3):
    """A: list[bytes]; reads whose first lattice hit is at an edge: the array on the last lattice seed it fits behind, the
    second copy ending at base L - 2, DR-to-DR distances on word boundaries, DRs at word starts; an N outside the array and an
    N inside a seed (it packs as 'A').  Only reads the oracle finds."""
    p = orc.Params(*pkey)
    s = shape(p, L)
    if not has_seed(p, L):
        return []
    rng = np.random.default_rng([seed, L] + list(pkey))
    bg, _ = backgrounds(rng, p, L, n_try)
    out = []
    for i in range(n_try):
        kind = ("late", "end", "word", "start")[i % 4]
        arr, dl = _array(rng, p, n_rep=int(rng.integers(2, 4)))
        if kind == "word":
            dists = [D for D in range(s.D0, s.D1 + 1) if D % 16 in (0, 1, 15)]
            D = int(rng.choice(dists)) if dists else s.D0
            if not (p.lowSpacerSize <= D - dl <= p.highSpacerSize):
                continue
            arr, dl = _array(rng, p, dr_len=dl, sp_lens=[D - dl] * 3, n_rep=int(rng.integers(2, 4)))
        if len(arr) > L - 1:
            arr = arr[:L - 1]
        room = L - 1 - len(arr)                                         # (a copy may not reach the read's last base)
        if kind == "late":
            at = s.skips * (min(s.searchEnd, room) // s.skips)
        elif kind == "end":
            at = room
        elif kind == "word":
            at = int(rng.choice([x for x in range(0, room + 1) if x % 8 == 0] or [0]))
        else:
            at = int(rng.choice([0, 1, s.skips] if s.skips <= room else [0]))
        if at < 0 or at > room:
            continue
        a = bg[i].copy()
        a[at:at + len(arr)] = arr
        r = a.tobytes()
        if orc.search_core(r, p)[0] != 1:
            continue
        out.append(r)
        if len(out) % 5 == 0:                                           # an N outside the array ...
            b = bytearray(r)
            b[L - 1 if at + len(arr) < L - 1 else 0] = ord("N")
            if at > 0 or at + len(arr) < L - 1:
                out.append(bytes(b))
        if len(out) % 7 == 0:                                           # ... and one inside the first lattice seed of the array
            b = bytearray(r)
            j = s.skips * (-(-at // s.skips))
            b[min(L - 1, j + int(rng.integers(0, s.w)))] = ord("N")
            out.append(bytes(b))
    return [r for r in out if orc.search_core(r, p)[0] == 1]


def _record(read, p):
    return orc.search_core(read, p)


@functools.lru_cache(maxsize=None)
def class_switch_set(pkey, L, target=200, max_cand=30000, seed=4):
    """S: (reads, the same reads without the decoy, candidates tried).  A decoy (one lattice seed copied D0 .. D1 on, no DR around it: the oracle rejects the
    candidate and moves its seed loop to ss[last] - 1) and a real array behind the decoy's copy.  Kept iff (a) the oracle finds
    the read after at least one class switch and (b) its record differs from the record of the same read with the decoy's
    copy replaced by the original bases."""
    p = orc.Params(*pkey)
    s = shape(p, L)
    rng = np.random.default_rng([seed, L] + list(pkey))
    out, twins, tried = [], [], 0
    while len(out) < target and tried < max_cand:
        bg, _ = backgrounds(rng, p, L, 500)
        for a0 in bg:
            if len(out) >= target or tried >= max_cand:
                break
            tried += 1
            arr, _ = _array(rng, p, n_rep=int(rng.integers(2, 5)), mut=int(rng.integers(0, 3)))
            room = L - 1 - len(arr)                                     # (the array ends before the read's last base)
            jd = s.skips * int(rng.integers(0, max(1, min(4, s.searchEnd // s.skips))))
            hi = min(dmax(s, jd), room - jd - s.w)                      # (the decoy's copy ends before the array starts)
            if hi < s.D0:
                continue
            dd = int(rng.integers(s.D0, hi + 1))
            lo_at = jd + dd + s.w
            at = int(rng.integers(lo_at, min(room, lo_at + 3 * s.skips + 24) + 1))
            plain = a0.copy()
            plain[at:at + len(arr)] = arr
            dec = plain.copy()
            _plant(dec, jd, jd + dd, s.w)
            r = dec.tobytes()
            class_switches(reset=True)
            rec = _record(r, p)
            n_sw = class_switches()[1]
            if rec[0] != 1 or n_sw < 1:
                continue
            if _record(plain.tobytes(), p) == rec:
                continue
            out.append(r)
            twins.append(plain.tobytes())
    return out, twins, tried
