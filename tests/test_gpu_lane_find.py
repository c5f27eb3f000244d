"""The lane kernel's packed seed find (crass_amd/csrc/lane_find.h, ln_find of survivor_lanes.hip) on designed reads: sets of 256 .. 512
reads — one block to two blocks of k_survivor_lanes — through the whole pipeline against the oracle, field by field, and a
second time in a fresh child process with CRASS_LANE_FIND_SERIAL=1 (the one-candidate-per-step loop), which must give the
same.  The find's own rule, candidate by candidate, is tests/test_lane_find_host.py's business; here its windows sit where
the kernel puts them:

  edge pairs      one exact copy of a lattice seed exactly at beginSearch, one base behind it, at the last candidate and one
                  before it, the window clipped by the read's end or not (edge_reads.positive_set) — chance 8-mers, whose
                  rejected candidate sends the lane off the lattice with several finds up to searchEnd
  one past        the copy one base past the last candidate: ending with the read's last base (the hint bit is set — the hints
                  ignore the clamp — and the find must not see it), and at D1 + 1 behind a decoy (no hints off the lattice)
  off the lattice behind a decoy: copies of an off-lattice seed at beginSearch, at the last candidate and one past it
  poly-A          a poly-A seed whose clipped window ends in A's: the zero bases past the read's end are not text
  arrays          real two- and three-repeat arrays at the edges (array_set), arrays behind a decoy (class_switch_set)

The reads above are chance 8-mers or arrays found through a candidate in the middle of a window: their records do not change
when a window's first or last candidate is lost.  What pins the window's edges — ln_find's candidate count, its clamps and
its chunk loop exist in survivor_lanes.hip only — are the EDGE ARRAYS (edge_arrays): real arrays in which EVERY seed of
the repeat has its only copy at one edge of its window, so the read is found iff that candidate is:

  first           THREE repeats, DR = lowDR, spacers = lowSp: the copy exactly at beginSearch and the third copy past the
                  window, anywhere in the read and at its end (clipped windows of a few candidates).  Three, because
                  qcFoundRepeats measures the one spacer of two repeats a base short: lowDR + lowSp + 1 is the nearest pair
                  it accepts, the SECOND candidate.  Not at 100 bases, which hold no three repeats
  last            DR = highDR, spacer = highSp: the copy is the last candidate; also with the array's last base at L - 2, the
                  window's end exactly the clamp L - 1.  Only where the read holds DR + spacer + DR (not at 100 bases) and
                  where qcFoundRepeats can accept the pair (|spacer - DR| <= 30: not under -S 90, whose last acceptable
                  distance, highDR + highDR + 30, lies inside the second chunk and is used instead)
  chunk edges     -S 90: the copy at the last candidate of the find's first chunk and at the first of its second

scanRight's window (24 bases either side of the expected place, clamped at L) has no such read: a third copy that is only
found at that window's edge is a stub at the read's end, and extendPreRepeat drops a repeat from the vote for every column
past it — the candidate ends at nine bases and is rejected with or without the third copy.

Every such read is kept only if the oracle's record IS the array (edge_arrays checks the start/stops).  Checked once against
an oracle whose searchCore window was moved by one base (not part of the suite: the oracle is a yardstick):
  first candidate dropped     every set's records change but L100's
  last candidate dropped      every set's but L100's, S90's and S90_L400's: no accepted array can depend on it there (above)
  a chunk-edge candidate lost (the last of chunk one, the first of chunk two)     both -S 90 sets' change
  one candidate more, in front of the first or past the last     nothing changes anywhere, and cannot: D0 - 1 is a spacer
                              below lowSp or a repeat below lowDR, D1 + 1 one above highSp or highDR, and a clipped window's
                              one-past copy leaves no room for a repeat.  These two are tests/test_lane_find_host.py's, on
                              find_packed and a copy of the chunk loop.

QC ARRAYS (qc_arrays) pin ln_qc, the in-lane qcFoundRepeats that the pooled tests do not take: arrays of four to seven repeats
(251 and 400 bases) and, under -S 90, spacers beyond 64 bases with two, three and four repeats — the similarity tests' one
site in its three modes, the per-base distance loops, the float averages in the reference's order.  The POOLED QC of two and
three repeats (qc_pool_begin_queued .. qc_pool_end), the extension and the orientation are tests/test_gpu_lane_sets.py's, on
the twin pairs of tests/lane_sets.py.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import edge_reads as E
from tests import orc
from tests.parity import assert_same_pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# id: (options, read length).  w7 / w9: another code width, w9 the serial route (18 bits: no two codes per register);
# S90: a window of 89 candidates, two chunks of the packed find
CASES = {
    "L150": ({}, 150),
    "L100": ({}, 100),
    "L251": ({}, 251),
    "w7": (dict(searchWindowLength=7), 150),
    "w9": (dict(searchWindowLength=9), 150),
    "S90": (dict(highSpacerSize=90), 251),
    "L400": ({}, 400),
    "S90_L400": (dict(highSpacerSize=90), 400),
}


def _params(ca, kw):
    p = ca.default_params(**kw)
    return p, orc.Params(p.lowDRsize, p.highDRsize, p.lowSpacerSize, p.highSpacerSize, p.searchWindowLength, p.minNumRepeats,
                         p.kmer_clust_size)


def designed(op, L, seed=18):
    """the reads edge_reads does not make: list[bytes]"""
    s = E.shape(op, L)
    rng = np.random.default_rng([seed, L] + list(E.key(op)))
    bg, _ = E.backgrounds(rng, op, L, 400)
    bg = iter(bg)
    out = []
    lattice = list(range(0, s.searchEnd + 1, s.skips))
    # the copy ends with the read's last base: p + w == L, one past the last candidate of the clipped window (end = L - 1)
    for j in lattice:
        d = L - s.w - j
        if s.D0 <= d <= s.D1:
            a = next(bg).copy()
            E._plant(a, j, j + d, s.w)
            out.append(a.tobytes())
    # a poly-A seed next to the read's end, the read ending in 1 .. w - 1 A's behind a C
    for j in lattice[-4:]:
        for tail in range(1, s.w):
            if j + s.D0 + s.w > L - tail - 1:
                continue
            a = next(bg).copy()
            a[j:j + s.w] = ord("A")
            a[L - tail - 1] = ord("C")
            a[L - tail:] = ord("A")
            out.append(a.tobytes())
            b = a.copy()                                   # ... and with a real poly-A copy as the last candidate
            b[L - 1 - s.w - 1] = ord("C")
            b[L - 1 - s.w:L - 1] = ord("A")
            out.append(b.tobytes())
    # behind a decoy (seed 0 copied D0 on: rejected, the loop goes on at D0 + w - 2 + skips, off the lattice and without hints)
    j1 = s.D0 + s.w - 2 + s.skips
    for js in range(j1, s.searchEnd + 1, s.skips):
        dm = E.dmax(s, js)
        for d in sorted({s.D0, s.D0 + 1, dm - 1, dm, dm + 1}):
            if d < s.D0 or js + d + s.w > L:
                continue
            for with_dr in (False, True):
                a = next(bg).copy()
                E._plant(a, 0, s.D0, s.w)
                if with_dr:                                # the seed inside a repeat of lowDR bases, so that a find shows in the record
                    n = int(op.lowDRsize)
                    lo = max(js - 3, s.D0 + s.w)
                    if lo + d + n > L:
                        continue
                    a[lo + d:lo + d + n] = a[lo:lo + n]
                else:
                    E._plant(a, js, js + d, s.w)
                out.append(a.tobytes())
    return out


def _repeats(rng, a, at, dr_len, sp_lens, stub=0):
    """DR (spacer DR)* at `at` of the read a (in place; stub > 0: only that many bases of the last copy), the bases in front of
    the copies pairwise different, and the bases behind them: no column next to the repeat gets two votes"""
    dr = E._rand(rng, dr_len)
    parts = [dr]
    for sl in sp_lens:
        parts += [E._rand(rng, sl), dr]
    if stub:
        parts[-1] = dr[:stub]
    arr = np.concatenate(parts)
    a[at:at + len(arr)] = arr
    starts = [at]
    for sl in sp_lens:
        starts.append(starts[-1] + dr_len + sl)
    front = list(rng.permutation(4))                            # (at most four copies)
    behind = list(rng.permutation(4))
    for k, st in enumerate(starts):
        if st > at:
            a[st - 1] = E.LETTERS[front[k]]
        elif st > 0:
            front[0] = int(E._CODE[a[st - 1]]); front[1:] = [c for c in range(4) if c != front[0]]
        if k + 1 < len(starts):
            a[st + dr_len] = E.LETTERS[behind[k]]
    last = starts[-1] + (stub or dr_len)
    if last < len(a) and not stub:
        a[last] = E.LETTERS[behind[len(starts) - 1]]
    return starts


def edge_arrays(op, L, seed=19):
    """{kind: [reads]}: see the module's text.  Kept only if the oracle's record is exactly the planted array."""
    s = E.shape(op, L)
    rng = np.random.default_rng([seed, L] + list(E.key(op)))
    lo_dr, hi_dr, lo_sp, hi_sp = int(op.lowDRsize), int(op.highDRsize), int(op.lowSpacerSize), int(op.highSpacerSize)
    # (two repeats: qcFoundRepeats measures the spacer one base short, so lowSp itself is accepted between THREE repeats only)
    plans = [("first", lo_dr, [lo_sp, lo_sp])]
    if hi_sp - 1 - hi_dr <= 30:
        plans.append(("last", hi_dr, [hi_sp]))
    else:
        plans.append(("last_accepted", hi_dr, [hi_dr + 30]))
    chunk = 64 - s.w + 1
    if s.D1 - s.D0 + 1 > chunk:                                  # the find's chunk loop: offsets chunk - 1 and chunk
        for name, d in (("chunk_last", s.D0 + chunk - 1), ("chunk_first", s.D0 + chunk)):
            dr = min(hi_dr, d // 2)
            plans.append((name, dr, [d - dr]))
    bg = iter(E.backgrounds(rng, op, L, 400)[0])
    out = {}
    for kind, dr, sps in plans:
        span = dr * (len(sps) + 1) + sum(sps)
        keep = out.setdefault(kind, [])
        if span > L - 1:
            continue
        room = L - 1 - span                                     # (the array ends before the read's last base)
        starts = sorted(set(range(0, min(room, 17) + 1)) | {room, max(0, room - 1), max(0, room - 7), room // 2})
        for at in starts:
            a = next(bg).copy()
            st = _repeats(rng, a, at, dr, sps)
            r = a.tobytes()
            if orc.search_core(r, op)[:2] == (1, [x for q in st for x in (q, q + dr - 1)]):
                keep.append(r)
    return out


def qc_arrays(op, L, seed=20):
    """{kind: [reads]} for ln_qc: four to seven repeats; strings beyond 64 bases (where the options allow a spacer that long)"""
    rng = np.random.default_rng([seed, L] + list(E.key(op)))
    bg = iter(E.backgrounds(rng, op, L, 300)[0])
    out = {"four_and_more": [], "beyond_64": []}
    hi_sp = int(op.highSpacerSize)
    for i in range(120):
        n_rep = 4 + i % 4
        arr, dl = E._array(rng, op, n_rep=n_rep, mut=i % 3)
        if len(arr) > L - 1:
            continue
        a = next(bg).copy()
        at = int(rng.integers(0, L - len(arr)))
        a[at:at + len(arr)] = arr
        r = a.tobytes()
        rec = orc.search_core(r, op)
        if rec[0] == 1 and len(rec[1]) >= 8:
            out["four_and_more"].append(r)
    if hi_sp > 64:
        for i in range(120):
            n_rep = 2 + i % 3
            dr = int(rng.integers(max(int(op.lowDRsize), 66 - 30), int(op.highDRsize) + 1))
            sps = [int(rng.integers(65, min(hi_sp, dr + 30) + 1)) for _ in range(n_rep - 1)]
            arr, _ = E._array(rng, op, dr_len=dr, sp_lens=sps, n_rep=n_rep, mut=i % 2)
            if len(arr) > L - 1:
                continue
            a = next(bg).copy()
            at = int(rng.integers(0, L - len(arr)))
            a[at:at + len(arr)] = arr
            r = a.tobytes()
            rec = orc.search_core(r, op)
            if rec[0] == 1 and max(rec[1][k + 2] - rec[1][k + 1] - 1 for k in range(0, len(rec[1]) - 2, 2)) > 64:
                out["beyond_64"].append(r)
    return out


def case_reads(cid):
    kw, L = CASES[cid]
    op = orc.Params.default(**kw)
    key = E.key(op)
    P = E.positive_set(key, L)
    A = E.array_set(key, L, n_try=200)
    S = E.class_switch_set(key, L, target=60, max_cand=4000)[0] if L >= 150 else []
    D = designed(op, L)
    EA = edge_arrays(op, L)
    QA = qc_arrays(op, L) if L >= 251 else {}
    edge = [r for k in sorted(EA) for r in EA[k][:24]]
    qc = [r for k in sorted(QA) for r in QA[k][:40]]
    reads = edge + qc + D[:120] + P[:100] + A[:80] + S[:40]
    spare = P[100:] + A[80:] + D[120:]                          # (a set is one block of the kernel at least)
    reads += spare[:max(0, 256 - len(reads))]
    # (order mixed, so that a wave holds reads of every kind; the same in parent and child)
    order = np.random.default_rng(len(reads)).permutation(len(reads))
    kinds = dict(designed=min(len(D), 120), edge_pairs=min(len(P), 100), arrays=min(len(A), 80), decoys=min(len(S), 40), spare=len(reads) - len(edge) - len(qc) - min(len(D), 120) - min(len(P), 100) - min(len(A), 80) - min(len(S), 40))
    kinds.update({"edge_" + k: min(len(v), 24) for k, v in EA.items()})
    kinds.update({"qc_" + k: min(len(v), 40) for k, v in QA.items()})
    return [reads[i] for i in order][:512], kinds


def digest(g):
    h = hashlib.sha256()
    n = int(g.n_pass1) + int(g.n_pass2)
    for a in (g.rec_read[:n], g.rec_lowlexi[:n], g.rec_nss[:n], g.rec_token[:n], g.rec_replen[:int(g.n_pass1)]):
        h.update(np.ascontiguousarray(a).tobytes())
    for k in range(n):
        h.update(repr(g.ss(k)).encode())
    for t in list(g.tokens) + list(g.patterns):
        h.update(bytes(t) + b"\n")
    return h.hexdigest()


def run_case(cid):
    """one set through the pipeline against the oracle; prints one JSON line with the result's digest"""
    import crass_amd as ca
    ca.load()
    kw, L = CASES[cid]
    p, op = _params(ca, kw)
    reads, kinds = case_reads(cid)
    assert 256 <= len(reads) <= 512, (cid, len(reads), kinds)
    # the reads that pin the window's edges and ln_qc are really there (their kinds: the module's text)
    if L >= 150:
        assert kinds["edge_first"] >= 10, kinds
        assert kinds.get("edge_last", 0) >= 6 or kinds.get("edge_last_accepted", 0) >= 10, kinds
    if "S90" in cid:
        assert kinds["edge_chunk_last"] >= 10 and kinds["edge_chunk_first"] >= 10, kinds
        assert kinds["qc_beyond_64"] >= 10, kinds
    if L >= 251:
        assert kinds["qc_four_and_more"] >= 10, kinds
    g = ca.search_pipeline(reads, params=p)
    ref = orc.pipeline(reads, params=op)
    assert_same_pipeline(g, ref)
    assert g.counters["n_filter_survivors"] >= 200          # (the lanes of one block and more hold a read)
    assert 20 <= g.n_pass1 < len(reads)                     # found and rejected reads side by side
    line = dict(case=cid, n=len(reads), kinds=kinds, survivors=int(g.counters["n_filter_survivors"]), n_pass1=int(g.n_pass1),
                n_pass2=int(g.n_pass2), serial=os.environ.get("CRASS_LANE_FIND_SERIAL", ""), digest=digest(g))
    print(json.dumps(line), flush=True)
    return line


@pytest.mark.parametrize("cid", list(CASES))
def test_designed_reads_packed_and_serial(cid):
    assert "CRASS_LANE_FIND_SERIAL" not in os.environ
    here = run_case(cid)
    env = dict(os.environ, CRASS_LANE_FIND_SERIAL="1")
    code = "from tests.test_gpu_lane_find import run_case; run_case(%r)" % cid
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    there = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert there["serial"] == "1" and there["case"] == cid
    assert there["digest"] == here["digest"] and there["n_pass1"] == here["n_pass1"] and there["n_pass2"] == here["n_pass2"]
