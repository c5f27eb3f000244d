"""The designed twin pairs of tests/lane_sets.py on the CPU: every kept pair's two written-down answers are the oracle's and differ,
every recorded component value (orc_levenshtein, orc_similarity, orc_is_low_complexity, orc_extend_pre_repeat,
orc_qc_found_repeats) lies on the side of its edge that the design states, the named grid cells are populated, and every set is
what tests/test_gpu_lane_sets.py takes it for.  The minimum counts are conditions the oracle alone meets.

Kept pairs as test_counts prints them, read length : pairs (a pair is two reads one step apart; the designer redraws until
orc_levenshtein hits the target distance, so nearly every planned pair survives; sim2 plans 69 pairs a length where all fit):

    sim2            defaults 100: 16, 150: 180, 251: 69, 400: 69, 512: 69;  S20_60, D64S70, D75 at 251: 69 each
    words           defaults 150: 18;  D64S70 251: 12
    transposition   defaults 150: 6, 251: 6
    sim3            defaults 150: 8, 200: 31, 251: 40, 400: 40, 512: 38;  S20_60 251: 39;  D64S70 251: 40
    lengths         defaults 150: 12, 251: 24, 400: 24;  S20_60 251: 6
    low_complexity  defaults 128: 20, 150: 24 (every length x letter)
    extend2         defaults 150: 18, 177: 22, 251: 22;  D75 251: 32
    votes           defaults 251: 24, 333: 36, 400: 48, 512: 48
    chain           defaults 251: 6, 400: 6
    orientation     defaults 129: 23, 150: 29;  D75 251: 61
    second_round    defaults 251, 300, 400, 512: 16 each
    field_edges     defaults 497, 511, 512: 12 each
"""
import pytest

from tests import orc
from tests import lane_sets as S
from tests import walk_sets as W

CUT = 0.82


def one_base_apart(a, b):
    return len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1


def all_pairs():
    seen, out = set(), []
    for name in S.SETS:
        for pr in S.pairs_of(name):
            if id(pr) not in seen:
                seen.add(id(pr))
                out.append(pr)
    return out


def of_kind(kind):
    return [pr for pr in all_pairs() if pr.kind == kind]


def test_every_pair_is_the_oracles_and_differs():
    n = 0
    for pr in all_pairs():
        p = S.params(pr.draw)
        wa, wb = pr.a.want(), pr.b.want()
        assert wa != wb, pr.name
        assert W.oracle_record(pr.a, p) == wa and W.oracle_record(pr.b, p) == wb, pr.name
        n += 1
    assert n > 1000


def _sim2_like(pr):
    y = pr.why
    assert y["d_no"] == S.d_no(max(y["n"], y["m"])), pr.name
    # d_no is the cut: one below is above 0.82, d_no itself is not (the reference's float expression, through orc_similarity)
    assert y["lev"] == (y["d_no"] - 1, y["d_no"]), pr.name
    assert (S.lev(y["dr"], y["sp"][0]), S.lev(y["dr"], y["sp"][1])) == y["lev"]
    assert S.sim(y["dr"], y["sp"][0]) > CUT >= S.sim(y["dr"], y["sp"][1]), pr.name
    assert y["qc"] == (0, 1), pr.name
    assert len(y["dr"]) == y["n"] <= 64 and len(y["sp"][0]) == len(y["sp"][1]) == y["m"] <= 64


@pytest.mark.parametrize("kind", ["sim2", "words", "field_edges", "second_round"])
def test_similarity_twins_of_two_repeats(kind):
    """distance d_no - 1 | d_no, similarity above | not above the cut, the twins one base apart, nothing else differs"""
    prs = [pr for pr in of_kind(kind) if "d_no" in pr.why]
    for pr in prs:
        _sim2_like(pr)
        assert one_base_apart(pr.a.seq, pr.b.seq), pr.name
        assert pr.b.found and pr.b.replen == pr.why["n"]
        assert pr.a.found == (kind == "second_round")             # (there the rejected candidate's read holds the array behind it)
    if kind == "sim2":
        for L in (150, 251, 400, 512):
            mine = [pr for pr in prs if pr.L == L]
            assert len(mine) >= 24, (L, len(mine))
        full = [pr for pr in prs if pr.L == 251]
        cells = {(pr.why["n"], pr.why["m"], pr.why["mode"]) for pr in full}
        for n in S.SIM2_N:
            ms = {m for (n_, m, _) in cells if n_ == n}
            assert any(m > n for m in ms), n
            if n >= 31:
                assert any(m < n for m in ms) and n in ms, (n, ms)       # below, equal and above (below 28 the spacer bound forbids both)
            for m in ms:
                assert {mode for (n_, m_, mode) in cells if (n_, m_) == (n, m)} == set(S.MODES), (n, m)
        for n in (31, 32, 33):
            assert {(n, n, "first"), (n, n, "last"), (n, n, "spread")} <= cells
    if kind == "words":
        assert {(pr.draw, pr.why["n"], pr.why["m"]) for pr in prs} == {("defaults", 31, 31), ("defaults", 32, 32), ("defaults", 33, 33),
                                                                      ("D64S70", 63, 64), ("D64S70", 64, 64)}
    if kind == "field_edges":
        for L in (512, 511, 497):
            for back in (1, 2):
                mine = [pr for pr in prs if pr.L == L and pr.sub.startswith("ends_at_L-%d" % back)]
                assert len(mine) >= 4, (L, back)
                for pr in mine:
                    sp = pr.b.info["spans"]
                    assert sp[1][1] == L - back and sp[0][1] + 1 > 255 and sp[1][0] > 400         # s0 / t0 use their ninth bit
    if kind == "second_round":
        for pr in prs:
            a, b = pr.a.info["spans"], pr.b.info["spans"]
            assert a[0][0] > b[1][1] + 8 and pr.L in (251, 300, 400, 512), pr.name


def test_second_round_by_length():
    prs = [pr for pr in of_kind("second_round") if "d_no" not in pr.why]
    assert len(prs) >= 4
    for pr in prs:
        assert pr.why["qc"] == (0, 1) and pr.a.found and pr.b.found
        assert pr.a.info["spans"][0][0] > pr.b.info["spans"][1][1]


def test_transposition_twins():
    """the found twin's distance is d_no only because its swap (bases 0-1) counts two; counted one it would be d_no - 1, as the
    other twin's is, whose swap sits where the reference counts it one"""
    prs = of_kind("transposition")
    assert {pr.sub for pr in prs} == set(S.TRANSPOSITIONS) and len(prs) >= 4
    for pr in prs:
        y = pr.why
        assert y["lev"] == (y["d_no"] - 1, y["d_no"]) and y["free"] == (y["d_no"] - 1, y["d_no"] - 1), pr.name
        assert (S.lev(y["dr"], y["sp"][0]), S.lev(y["dr"], y["sp"][1])) == y["lev"]
        assert (S.osa_free(y["dr"], y["sp"][0]), S.osa_free(y["dr"], y["sp"][1])) == y["free"]
        assert S.sim(y["dr"], y["sp"][0]) > CUT >= S.sim(y["dr"], y["sp"][1]) and y["qc"] == (0, 1)
        assert y["sp"][1][:2] == y["dr"][1::-1] and sorted(y["sp"][0]) == sorted(y["sp"][1])        # the same bases, the swap moved
        assert not pr.a.found and pr.b.found


def test_sim3_twins():
    prs = of_kind("sim3")
    main = [pr for pr in prs if pr.L == 251 and pr.draw == "defaults"]
    assert len(main) >= 16
    for sub in S.SIM3:
        assert sum(pr.sub.startswith(sub) for pr in main) >= 4, sub
    assert {pr.why["n"] for pr in main} >= {24, 31, 32, 33, 40}
    for pr in prs:
        y = pr.why
        dn, sub = y["d_no"], pr.sub.rsplit("_n", 1)[0]
        assert dn == S.d_no(y["m"]) and y["qc"] == (0, 1) and not pr.a.found and pr.b.found, pr.name
        assert max(len(y["dr"]), y["m"]) <= 64
        ss = (S.sim(*y["a"]), S.sim(*y["b"]))
        rs = (S.sim(y["dr"], y["a"][0]), S.sim(y["dr"], y["b"][0]))
        if sub == "ss":
            assert y["lev_ss"] == (dn - 1, dn) and ss[0] > CUT >= ss[1] and max(rs) < 0.6, pr.name
        elif sub == "rs":                                         # the first test far below: only slot_b's result rejects the read
            assert y["lev_rs"] == (dn - 1, dn) and rs[0] > CUT >= rs[1] and max(ss) < 0.6, pr.name
        elif sub == "both_a":
            assert y["lev_ss"] == (dn - 1, dn) and ss[0] > CUT >= ss[1] and y["lev_rs"] == (dn, dn), pr.name
        else:
            assert y["lev_rs"] == (dn - 1, dn) and rs[0] > CUT >= rs[1] and dn <= min(y["lev_ss"]) <= dn + 1 and max(ss) <= CUT, pr.name


def test_length_twins():
    prs = of_kind("lengths")
    subs = {(pr.draw, pr.sub) for pr in prs}
    assert subs >= {("defaults", s) for s in ("two_low", "two_high", "three_short_first", "three_short_second", "three_long_first",
                                              "three_long_second", "three_s1_s2_13", "three_s2_s1_13")}
    assert subs >= {("S20_60", "two_rep_sp_31"), ("S20_60", "three_rep_sp_31")}
    for pr in prs:
        p = S.params(pr.draw)
        sa, sb = pr.why["sps"]
        assert sum(abs(x - y) for x, y in zip(sa, sb)) == 1 and pr.why["qc"] == (0, 1) and not pr.a.found and pr.b.found, pr.name
        n, lo, hi = pr.why["n"], int(p.lowSpacerSize), int(p.highSpacerSize)
        short = 1 if len(sb) == 1 else 0                           # two repeats: measured one base short
        m = [x - short for x in sb]
        assert lo <= min(m) and max(m) <= hi and abs(n - m[0]) <= 30 and (len(m) == 1 or abs(m[0] - m[1]) <= 12)
        edge = {"two_low": m[0] == lo, "two_high": m[0] == hi, "three_short_first": m[0] == lo, "three_short_second": m[-1] == lo,
                "three_long_first": m[0] == hi, "three_long_second": m[-1] == hi, "three_s1_s2_13": abs(m[0] - m[-1]) == 12,
                "three_s2_s1_13": abs(m[0] - m[-1]) == 12, "two_rep_sp_31": abs(n - m[0]) == 30, "three_rep_sp_31": abs(n - m[0]) == 30}
        assert edge[pr.sub], pr.name


def test_low_complexity_twins():
    prs = [pr for pr in of_kind("low_complexity") if pr.L == 150]
    assert {(pr.why["n"], pr.why["letter"]) for pr in prs} == {(n, x) for n in (23, 24, 32, 33, 40, 47) for x in "ACGT"}
    for pr in of_kind("low_complexity"):
        y = pr.why
        assert y["cut_off"] == int(y["n"] * 0.75) and y["count"] == (y["cut_off"] + 1, y["cut_off"]) and y["low"] == (1, 0)
        assert y["qc"] == (0, 1) and not pr.a.found and pr.b.found
        assert sum(x != z for x, z in zip(pr.a.seq, pr.b.seq)) == 2          # one base of either copy


def _seeds(r, p):
    """the seed spans the oracle's searchCore hands to extendPreRepeat for the designed array: the first lattice seed inside the
    first repeat (a lead read: the repeat's last seed offset) and its copies"""
    sp = r.info["spans"]
    if r.info.get("lead"):
        j = sp[0][1] - 7
    else:
        j = -(-sp[0][0] // 8) * 8
    o = j - sp[0][0]
    return [(a + o, a + o + 7) for a, b in sp]


def test_extension_twins():
    for draw, L, need in (("defaults", 150, ()), ("defaults", 251, ("low_last", "high_last")),
                          ("D75", 251, ("low_last", "high_last", "chunk_right_63|64", "chunk_right_64|65", "chunk_left_63|64", "chunk_left_64|65", "chunk_76|75"))):
        prs = S.extend2(draw, L)
        subs = {pr.sub for pr in prs}
        assert subs >= {"%s_off%d" % (s, o) for s in ("low", "high") for o in (0, 4, 7)} | {"first_at_0|1", "first_at_1|2", "second_ends_at_L-1|2"} | set(need), (draw, L, subs)
        p = S.params(draw)
        for pr in prs:
            for r in (pr.a, pr.b):
                n, sp = r.info["n"], r.info["spans"]
                assert r.found == (int(p.lowDRsize) <= n <= int(p.highDRsize)), pr.name
                # orc_extend_pre_repeat on the seeds gives the designed repeat, whether searchCore then accepts its length or not
                assert S.extend(r.seq, _seeds(r, p), p) == (n, sp), pr.name
                assert S.qc(r.seq, sp, p) == 1
            if "chunk" in pr.sub and "76" not in pr.sub:
                runs = tuple(int(x) for x in pr.sub.rsplit("_", 1)[1].split("|"))
                assert (pr.a.info["n"] - 8, pr.b.info["n"] - 8) == runs
                lead = bool(pr.a.info["lead"])
                assert lead == ("left" in pr.sub)                   # the whole run on one side of the seed
            if pr.sub.startswith("second_ends"):
                assert (pr.a.info["spans"][1][1], pr.b.info["spans"][1][1]) == (L - 1, L - 2)
            if pr.sub.startswith("first_at"):
                assert pr.b.info["spans"][0][0] - pr.a.info["spans"][0][0] == 1 and pr.a.info["spans"][0][0] in (0, 1)


def test_vote_twins():
    prs = S.votes("defaults", 400)
    subs = {pr.sub for pr in prs}
    for n_rep in (3, 4, 5, 7):
        assert subs >= {"n%d_%s_%s" % (n_rep, side, x) for side in ("left", "right") for x in "ACGT"}
        assert subs >= {"n%d_%s" % (n_rep, s) for s in ("cut_whole|1", "cut_1|3", "first_at_0", "shortest_second|first")}
    assert {pr.sub[:2] for pr in S.votes("defaults", 251)} == {"n3", "n4"}
    p = S.params("defaults")
    for pr in prs + S.votes("defaults", 251):
        for r in (pr.a, pr.b):
            sp = r.info["spans"]
            assert r.found and len(sp) == pr.why["n_rep"]
            o = (-sp[0][0]) % 8 if "first_at_0" not in pr.sub and "cut" not in pr.sub else None
            if o is not None:                                       # (the other two: the designed spans are clamped or cut)
                assert S.extend(r.seq, [(a + o, a + o + 7) for a, b in sp], p)[1] == sp, pr.name
        if "_left_" in pr.sub or "_right_" in pr.sub:
            side, x = pr.sub.split("_")[1:]
            cols = []
            st = [a for a, b in pr.a.info["spans"]]                   # (the twins share the layout; b's spans hold the column)
            for r in (pr.a, pr.b):
                cols.append([r.seq[s - 1] if side == "left" else r.seq[s + 26] for s in st])
            k = pr.why["cut_off"]
            assert cols[0].count(ord(x)) == k - 1 and cols[1].count(ord(x)) == k, (pr.name, cols)
            assert max(map(cols[0].count, b"ACGT")) < k
            assert (pr.a.replen, pr.b.replen) == (26, 27)
        if "cut_whole|1" in pr.sub:
            assert (pr.a.replen, pr.b.replen) == (26, 26) and pr.b.info["spans"][-1][1] - pr.b.info["spans"][-1][0] == 24
        if "cut_1|3" in pr.sub:
            assert (pr.a.replen, pr.b.replen) == (26, 24) and pr.b.info["spans"][-1][1] == pr.L - 1
        if "first_at_0" in pr.sub:
            assert pr.a.info["spans"][0][0] == pr.b.info["spans"][0][0] == 0 and (pr.a.replen, pr.b.replen) == (26, 27)


def test_chain_twins():
    for L in (251, 400):
        prs = S.chain("defaults", L)
        assert {pr.sub for pr in prs} == {"cand+25|24", "cand-25|24"}
        for pr in prs:
            sa, sb = pr.why["sps"]
            assert abs(sa[1] - sa[0]) == 25 and abs(sb[1] - sb[0]) == 24 and pr.b.found and len(pr.b.ss) == 8
            assert len(pr.a.ss) == (4 if pr.a.found else 0)


def test_orientation_twins():
    """the twin is the read's reverse complement: the same DR string, the other flag (a palindrome: flag 0 twice), and start/stops
    that are each other's mirror image before pass 1 turns the flagged-0 read round: the two records hold the same list"""
    prs = of_kind("orientation")
    drops = {pr.why["drop"] for pr in prs}
    assert drops == {">=64", "<64", "0", "bytes"}
    for pr in prs:
        a, b, y = pr.a, pr.b, pr.why
        L = pr.L
        assert b.seq == W.revcomp(a.seq) and a.found and b.found and a.replen == b.replen == y["n"]
        d = y["dr"]
        if y["first_diff"] is None:
            assert d == W.revcomp(d) and (a.low, b.low) == (0, 0)
            assert a.ss == [L - 1 - x for x in reversed(b.ss)] and a.ss != b.ss
        else:
            k = y["first_diff"]
            rc = W.revcomp(d)
            assert d[:k] == rc[:k] and (d[k] < rc[k]) == y["lower"]
            assert (a.low, b.low) == ((1, 0) if y["lower"] else (0, 1)) and a.ss == b.ss
    cells = {(pr.draw, pr.why["n"], pr.why["first_diff"], pr.why["lower"]) for pr in prs}
    for n in (23, 31, 32, 33, 47):
        for k in sorted({0, 15, 16, 31, 32, (n - 1) // 2} & set(range((n + 1) // 2))):
            assert {("defaults", n, k, True), ("defaults", n, k, False)} & cells, (n, k)
    for n in (63, 64, 65, 66, 70, 75):
        for k in sorted({0, 15, 16, 31, 32, (n - 1) // 2} & set(range((n + 1) // 2))):
            assert {("D75", n, k, True), ("D75", n, k, False)} <= cells, (n, k)
    assert {(pr.draw, pr.why["n"]) for pr in prs if pr.why["first_diff"] is None} >= {("defaults", 24), ("defaults", 32), ("defaults", 46), ("D75", 64)}
    assert sum(pr.why["at"] == 0 for pr in prs) >= 10                 # the pick rule with the first repeat at base 0


@pytest.mark.parametrize("name", S.SETS)
def test_the_sets(name):
    reads = S.the_set(name)
    p = S.params(S.draw_of(name))
    assert 256 <= len(reads) <= 1024
    lens = {r.L for r in reads}
    if name in S.PLANS:
        assert lens == {S.PLANS[name][1]}
    elif name == "ragged":
        assert min(lens) >= 100 and max(lens) <= 512 and {511, 497} <= lens and len(lens) >= 8
    res = orc.pipeline([r.seq for r in reads], params=p)
    assert res.error == 0
    positives = [i for i, r in enumerate(reads) if r.found]
    assert 0 < len(positives) and res.n_pass1 == len(positives) and res.rec_read[:res.n_pass1].tolist() == positives
    for k, i in enumerate(positives):
        r = reads[i]
        assert (int(res.rec_lowlexi[k]), int(res.rec_replen[k]), res.ss(k)) == (r.low, r.replen, r.ss), r.name
    if name in S.POOLS:
        assert len(reads) == len(positives) == S.POOLS[name]
        assert all(len(r.ss) == 6 for r in reads)
        assert all((r.replen <= 32) == (i % 2 == 0) for i, r in enumerate(reads))
    else:
        assert len(positives) < len(reads)                              # accepted and rejected reads side by side
        designed = [r for r in reads if r.kind != "background"]
        assert len(designed) >= 100
        for at in range(0, len(reads) - 63, 64):                        # every wave of a block in slot order holds several kinds
            assert len({r.kind for r in reads[at:at + 64]} - {"background"}) >= 2, (name, at)
    # no compared string beyond 64 bases, so the pool takes every test of two and three repeats — but under -D 75, whose repeats
    # of 65 .. 76 bases ln_qc takes in the lane; there the spacers stay at 64 or fewer (only a pair BOTH beyond 64 is handed over)
    for r in reads:
        sp = r.info.get("spans")
        if sp and len(sp) <= 3:
            short = 1 if len(sp) == 2 else 0                        # (the one spacer of two repeats is measured a base short)
            assert max(sp[k + 1][0] - sp[k][1] - 1 - short for k in range(len(sp) - 1)) <= 64, r.name
            assert max(b - a + 1 for a, b in sp) <= (76 if name == "D75" else 64), r.name


def test_counts():
    rows = {}
    for pr in all_pairs():
        rows[(pr.kind, pr.draw, pr.L)] = rows.get((pr.kind, pr.draw, pr.L), 0) + 1
    print("%-16s %-9s %4s %5s" % ("kind", "draw", "L", "pairs"))
    for (kind, draw, L), n in sorted(rows.items()):
        print("%-16s %-9s %4d %5d" % (kind, draw, L, n))
    kinds = {k for k, _, _ in rows}
    assert kinds == {"sim2", "words", "transposition", "sim3", "lengths", "low_complexity", "extend2", "votes", "chain", "orientation",
                     "second_round", "field_edges"}
    assert S.d_no(26) == 5 and S.d_no(32) == 6 and S.d_no(47) == 9 and S.d_no(50) == 9 and S.d_no(64) == 12
    # d_no by the definition, on the oracle's own similarity: a pair of strings d apart has similarity 1 - d / max
    for mx in (26, 32, 33, 47, 50, 64):
        a = b"A" * mx
        d = S.d_no(mx)
        assert S.sim(a, b"C" * (d - 1) + a[d - 1:]) > CUT >= S.sim(a, b"C" * d + a[d:])
