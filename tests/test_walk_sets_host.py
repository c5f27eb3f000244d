"""The designed reads of tests/walk_sets.py on the CPU: the restated light walk against the oracle (the yardstick), every read's
written-down answer against orc.search_core and orc.pipeline (the design), and the proof that a read's answer hangs on the edge
it is named after — the kind's mutant of the restatement loses it, or chain()'s record shows the mask edge (the dependence).
test_gpu_long_walk.py runs the same sets through the kernels.

Kept reads and mutant flips per kind and option draw, as test_counts prints them (conditions, asserted there):

    kind             draw      kept  found  flip        kind             draw      kept  found  flip
    batch            defaults    14     14    14        any              d15         30     26    26
    back_to_lattice  defaults    10     10    10        lengths          defaults     5      5     -
    third            n3          72     36    24        dense            defaults    46     38    36
    extend           defaults    33     27    27        dense            n3          24     12     8
    extend           D75         58     49    49        dense            w7          44     36    36
    any              w7          48     44    44        votes            defaults    70     70     -
    any              d20_D40     48     44    44        masks            defaults    31     31     -

(found but no flip: the reads whose design claims no dependence, named in walk_sets' text: third/ends_at_L and the two exception
reads.  masks: every label of MASK_LABELS on 8 reads at least.)
"""
import numpy as np
import pytest

from tests import orc
from tests import edge_reads as E
from tests import walk_sets as W

LIGHT = sorted(W.LIGHT_SETS)
WAVE = sorted(W.WAVE_SETS)
TWO = ("low_right_only", "low_both", "low_left_only", "high", "low-1", "high+1", "first_at_0", "first_at_1", "first_at_2",
       "second_ends_at_L-1", "second_ends_at_L-2")
CHUNKS = tuple("chunk_%s_%d" % (side, n) for n in (72, 73, 74, 75) for side in ("right", "left")) + ("chunk_76",)
BATCH_ANY = ("batch_w63", "batch_w64", "batch_w127", "batch_w128", "batch_last")
THIRD = ("cand+24", "cand-24", "cand+25", "cand-25", "ends_at_L", "minb")
# the sub-cases every set must hold (a read that `kept` drops must not take its sub-case with it)
SUBS = {
    ("batch", "defaults"): ("w0_behind_j", "w0_end", "w63", "w64", "w127", "w128", "last"),
    ("back_to_lattice", "defaults"): tuple("class%d" % c for c in range(1, 8)),
    ("third", "n3"): THIRD,
    ("extend", "defaults"): TWO,
    ("extend", "D75"): TWO + CHUNKS,
    ("any", "w7"): BATCH_ANY + TWO + ("off_lattice",),
    ("any", "d20_D40"): BATCH_ANY + TWO + ("off_lattice",),
    ("any", "d15"): BATCH_ANY + tuple(x for x in TWO if x != "low_both"),        # (a lattice of every base: no middle seed first)
    ("lengths", "defaults"): ("L2049", "L12225", "L12287", "L12288", "L12289"),
    ("dense", "defaults"): TWO + ("exception_N", "background"),
    ("dense", "n3"): THIRD + ("background",),
    ("dense", "w7"): TWO + ("background",),
}
NO_FLIPS = {"lengths"}                  # kinds without a slip of their own (walk_sets' text says why)
FIXED_LISTS = {"lengths", "votes"}      # a fixed list of positions: every listed case present instead of 8 reads


def acgt(r):
    return not (set(r.seq) - set(b"ACGT"))


def agrees(read, p):
    """the yardstick on one read: found => handed over; decided here => not found"""
    found = orc.search_core(read, p)[0] == 1
    verdict = W.light_walk(read, p)[0]
    assert verdict in (0, 7)
    assert not (found and verdict != 7) and not (verdict == 0 and found)
    return found, verdict


@pytest.mark.parametrize("draw", ["defaults", "n3", "w7", "d20_D40"])
def test_yardstick_on_random_reads(draw):
    """300 random reads of 2.1 .. 12.3 kbp (75 per draw), one in four with a planted array: chance decoys, class switches and
    arrays as they come"""
    p = W.params(draw)
    rng = np.random.default_rng([41] + list(E.key(p)))
    n_found = n_over = 0
    for i in range(75):
        L = int(rng.integers(2100, 12301))
        a = E._rand(rng, L)
        if i % 4 == 0:
            arr, _ = E._array(rng, p, n_rep=int(rng.integers(2, 6)), mut=int(rng.integers(0, 2)))
            at = int(rng.integers(0, L - len(arr)))
            a[at:at + len(arr)] = arr
        found, verdict = agrees(a.tobytes(), p)
        n_found += found
        n_over += verdict == 7
    print("%s: the oracle found %d of 75, the restatement handed over %d" % (draw, n_found, n_over))
    assert 10 <= n_found <= n_over


@pytest.mark.parametrize("kind,draw", LIGHT + WAVE)
def test_yardstick_and_design(kind, draw):
    """every read: the restatement agrees with the oracle; the written-down answer is orc.search_core's and orc.pipeline's"""
    reads = W.get(kind, draw)
    p = W.params(draw)
    for r in reads:
        assert W.oracle_record(r, p) == r.want(), r.name
        if acgt(r):
            found, verdict = agrees(r.seq, p)
            assert found == r.found, r.name
            if r.sub == "background":
                assert verdict == 0
    res = orc.pipeline([r.seq for r in reads], params=p)
    assert res.error == 0
    positives = [i for i, r in enumerate(reads) if r.found]
    assert res.n_pass1 == len(positives) and res.rec_read[:res.n_pass1].tolist() == positives
    for k, i in enumerate(positives):
        r = reads[i]
        assert (int(res.rec_lowlexi[k]), int(res.rec_replen[k]), res.ss(k)) == (r.low, r.replen, r.ss), r.name


def flips(kind, draw):
    reads = W.get(kind, draw)
    p = W.params(draw)
    return [r for r in reads if r.found and acgt(r) and r.mutant and W.light_walk(r.seq, p, mutant=r.mutant)[0] == 0]


@pytest.mark.parametrize("kind,draw", LIGHT)
def test_dependence_of_the_light_walk_reads(kind, draw):
    """every sub-case is there; the ONE slip a read is designed for (walk_sets.mutant_of: by kind and sub-case) loses every read
    whose design says so (Read.dep)"""
    reads = W.get(kind, draw)
    p = W.params(draw)
    assert {r.sub for r in reads} == set(SUBS[(kind, draw)])
    lost = {id(r) for r in flips(kind, draw)}
    for r in reads:
        if r.dep:
            assert id(r) in lost, (r.name, r.info)
    if kind == "batch":
        # the trace says where the array's candidate sat: behind one class switch, in the hint word of the read's name
        want = {"w0_behind_j": 0, "w0_end": 0, "w63": 63, "w64": 64, "w127": 127, "w128": 128}
        for r in reads:
            tr = []
            assert W.light_walk(r.seq, p, trace=tr)[0] == 7
            assert len(tr) == 2 and tr[0]["outcome"] == "rejected" and tr[0]["rho"] == 0 and tr[1]["rho"] != 0, r.name
            if r.sub == "last":
                assert tr[1]["j"] >> 6 == E.shape(p, r.L).searchEnd >> 6 and tr[1]["batch"] >= 128
            else:
                assert tr[1]["batch"] == want[r.sub], (r.name, tr[1])
            if r.sub == "w0_behind_j":
                assert tr[1]["j"] == tr[0]["pos"] + 8 - 2 + 8            # the first seed the walk looks at in its new class
    if kind == "back_to_lattice":
        for r in reads:
            tr = []
            W.light_walk(r.seq, p, trace=tr)
            assert [t["rho"] == 0 for t in tr] == [True, False, True] and tr[2]["outcome"] == "due for qc", r.name
    if kind == "third":
        for r in reads:
            tr = []
            v = W.light_walk(r.seq, p, trace=tr)[0]
            t = tr[0]
            if r.sub in ("cand+24", "cand-24"):
                assert v == 7 and t["third"] - t["cand"] == int(r.sub[4:]), r.name
            if r.sub == "ends_at_L":
                assert v == 7 and t["third"] + 8 <= r.L < t["cand"] + 8 + 24 and r.info["starts"][2] + r.replen == r.L, r.name
            if r.sub == "minb":
                assert v == 7 and t["third"] == t["minb"] > t["cand"] - 24 and not r.found, r.name
            if r.sub in ("cand+25", "cand-25"):
                assert v == 0 and not r.found
    if kind == "any" and E.shape(p, 3000).skips > 1:
        off = [r for r in reads if r.sub == "off_lattice"]
        assert len(off) >= 8
        bits = [W.hint_bits(r.seq, p) for r in off]
        for r, b in zip(off, bits):
            assert r.info["off"] and all(b[q] and q % E.shape(p, r.L).skips for q in r.info["off"]), r.name


def test_votes_show_their_columns():
    reads = W.get("votes", "defaults")
    seen = {(r.info["n_rep"], r.info["k"], r.info["place"]): r for r in reads}
    for n in W.VOTE_COUNTS:
        for k in (0, 1, 2):
            r = seen[(n, k, "middle")]
            # all copies but k agree: the column passes with no or one dissenter (two repeats: with none), and at three repeats
            # two dissenters are their own majority
            want = 1 if (k == 0 or (k == 1 and n >= 3) or (k == 2 and n == 3)) else 0
            assert r.info["ext"] == (want, want) and r.replen == 30 + 2 * want, r.name
            st = r.info["starts"]
            left, right = [r.seq[s - 1] for s in st], [r.seq[s + 30] for s in st]
            if (n, k) == (2, 2):
                assert left[0] != left[1] and right[0] != right[1]
            else:
                assert sum(c != ord("A") for c in left) == k and len(set(left)) <= 2, r.name
                assert sum(c != ord("G") for c in right) == k and len(set(right)) <= 2, r.name
            assert max(map([r.seq[s - 2] for s in st].count, b"ACGT")) <= -(-n // 4)        # the second column cycles
        for place, k in (("first_at_0", 0), ("first_at_0", 1), ("first_at_1", 0), ("ends_at_L-1", 0), ("ends_at_L-1", 1),
                         ("ends_at_L-2", 0), ("ends_at_L-2", 1)):
            r = seen[(n, k, place)]
            st = r.info["starts"]
            assert {"first_at_0": st[0] == 0, "first_at_1": st[0] == 1, "ends_at_L-1": st[-1] + 30 == r.L,
                    "ends_at_L-2": st[-1] + 30 == r.L - 1}[place], r.name
    assert len(reads) == len(seen) == len(W.VOTE_COUNTS) * 10


def test_masks_show_their_edges():
    reads = W.get("masks", "defaults")
    p = W.params("defaults")
    count = dict.fromkeys(W.MASK_LABELS, 0)
    for r in reads:
        st, off = r.info["starts"], r.info["off"]
        assert len(st) >= 70
        found, links = W.chain(r.seq, p, st[0] + off, st[1] + off)
        assert found == [s + off for s in st], r.name
        masked = [x for x in links if x["base"] is not None and x["found"] >= 0]
        assert masked == [dict(x, **y) for x, y in zip(masked, W.chain_plan(st, r.L, 8, 26, off))]      # the plan's bookkeeping
        assert any(x["rebuilt"] for x in masked[1:]), r.name                      # the chain passes a 4 096-base block
        # every window holds the repeat it finds and nothing else, but for the extra copies: those sit in the lane behind
        two = [x for x in masked if len(x["hits"]) > 1]
        assert all(x["hits"] == [x["lane"]] for x in masked if x not in two)
        assert all(x["hits"] == [x["k0"], x["k0"] + 1] and x["lane"] == x["k0"] and x["k1"] > x["k0"] for x in two)
        assert len(two) == len(r.info["extras"]) and all(r.seq[e:e + 8] == r.seq[st[0]:st[0] + 8] for e in r.info["extras"])
        assert ("both_lanes" in r.info["labels"]) == bool(two)
        lab = W._plan_labels(masked)
        assert lab == r.info["labels"] and lab
        for x in lab:
            count[x] += 1
        tr = []
        assert W.light_walk(r.seq, p, trace=tr)[0] == 7 and tr[-1]["j"] == st[0] + off and tr[-1]["outcome"] == "third"
    print("masks:", count)
    assert all(v >= 8 for v in count.values()), count


def test_counts():
    print("%-16s %-9s %5s %6s %5s" % ("kind", "draw", "kept", "found", "flip"))
    for kind, draw in LIGHT + WAVE:
        reads = [r for r in W.get(kind, draw) if r.sub != "background"]
        n_found = sum(r.found for r in reads)
        n_flip = len(flips(kind, draw)) if (kind, draw) in W.LIGHT_SETS and kind not in NO_FLIPS else None
        print("%-16s %-9s %5d %6d %5s" % (kind, draw, len(reads), n_found, "-" if n_flip is None else n_flip))
        if kind not in FIXED_LISTS:
            assert len(reads) >= 8 and n_found >= 8, (kind, draw)
        if n_flip is not None:
            assert n_flip >= 8, (kind, draw)
    assert sorted(r.L for r in W.get("lengths", "defaults")) == [2049, 12225, 12287, 12288, 12289]
    assert all(r.found for r in W.get("lengths", "defaults"))
    assert sorted({r.L for r in W.get("dense", "defaults")}) == [513, 1000, 2047, 2048]
    assert sum(not acgt(r) and r.found for r in W.get("dense", "defaults")) == 2


def test_turns():
    """8 192 + 64 reads; the designed slots, read by read; the rest as a whole"""
    reads = W.turns_set()
    p = W.params("defaults")
    assert len(reads) == W.TURN_SLOTS + 64 and 17e6 < sum(r.L for r in reads) < 19e6
    slots = W.turns_designed(reads)
    assert len(slots) == 64 and all((s < 64) != (s >= W.TURN_SLOTS) for s in slots)
    orders = set()
    for s in slots[:32]:
        a, b = reads[s], reads[s + W.TURN_SLOTS]
        assert {a.L > 12000, b.L > 12000} == {True, False} and {a.kind, b.kind} == {"batch", "extend"}
        orders.add(a.L > b.L)
    assert orders == {True, False}
    for s in slots:
        r = reads[s]
        assert W.oracle_record(r, p) == r.want() and agrees(r.seq, p)[0] == r.found
    assert all(2060 <= r.L <= 2200 for r in reads if r.sub == "background")
    assert not any(W.light_walk(r.seq, p)[0] for r in reads[64:W.TURN_SLOTS:37])          # a sample of the backgrounds
    res = orc.pipeline([r.seq for r in reads], params=p)
    positives = [s for s in slots if reads[s].found]
    assert res.error == 0 and res.rec_read[:res.n_pass1].tolist() == positives and len(positives) >= 48
