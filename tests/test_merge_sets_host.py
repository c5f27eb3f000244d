"""tests/merge_sets.py pinned on the CPU, before test_gpu_merge_sets.py trusts it: merge_reference against the oracle's
clusterDRReads + createNonRedundantSet (groups, the pattern list with its order, pattern groups) on the five golden inputs and on
the two synthetic token lists of test_merge_host.py; the host merge (crass_merge_create) against merge_reference on every designed
set, field by field; every designed token with the verdict it was designed for and none left out; every class the sets are named
for non-empty; the tier sets in their key ranges; every designed read with the verdict recruit_sets.find_singletons gives over the
reference's patterns."""
import os
import random

import numpy as np
import pytest

from tests import orc, fastx
from tests import merge_sets as ms
from tests import recruit_sets as rs

DATA = os.path.join(os.path.dirname(__file__), "golden", "data")
GOLDEN = ["Ill100.fx.gz", "CN_gDC.fa.gz", "front_offset_bug.fa.gz", "Ill.nr.miss.fa.gz", "poor_dr_ext.fa.gz"]


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


def assert_reference_is_the_oracle(res, k=6):
    assert res.error == 0 and res.n_groups >= 1
    groups, patterns, pat_group, dropped = ms.merge_reference(res.tokens, k)
    assert groups == res.groups
    assert patterns == res.patterns
    assert pat_group == res.pat_group.tolist()
    assert len(patterns) == 2 * (len(res.tokens) - len(dropped))


@pytest.mark.parametrize("fname", GOLDEN)
def test_reference_is_the_oracle_on_golden_inputs(fname):
    recs = fastx.read_fastx(os.path.join(DATA, fname))
    assert_reference_is_the_oracle(orc.pipeline([r[2] for r in recs], [r[0] for r in recs], do_pass2=False))


def test_reference_is_the_oracle_on_synthetic_tokens():
    """test_merge_host.py's first list: 60 000 synthetic reads, >= 40 groups"""
    import crass_amd as ca
    n = 60000
    asc = ca.unpack_ascii(ca.synth_packed(ca.synth_spec(read_len=150, crispr_per_million=100000), 0, n), 10, 150, n)
    res = orc.pipeline((asc, np.arange(0, (n + 1) * 150, 150, dtype=np.uint64)), do_pass2=False)
    assert res.n_groups >= 40
    assert_reference_is_the_oracle(res)


def variant_reads():
    """test_merge_host.py's second list: 120 DRs (some with an N) and their one-edit variants, > 2 500 tokens"""
    rng = random.Random(99)

    def rnd(n, alphabet=b"ACGT"):
        return bytes(rng.choice(alphabet) for _ in range(n))
    drs = [rnd(rng.randint(26, 38)) for _ in range(120)]
    for i in range(0, 120, 7):
        d = bytearray(drs[i]); d[rng.randint(3, len(d) - 4)] = ord("N"); drs[i] = bytes(d)
    seqs = []
    for _ in range(9000):
        d = bytearray(rng.choice(drs))
        if rng.random() < 0.7:
            k = rng.randrange(len(d))
            r = rng.random()
            if r < 0.7: d[k] = rng.choice(b"ACGT")
            elif r < 0.85: del d[k]
            else: d.insert(k, rng.choice(b"ACGT"))
        d = bytes(d)
        s = rnd(rng.randint(0, 12))
        while len(s) < 190:
            s += d + rnd(rng.randint(28, 38))
        seqs.append(s[:rng.randint(150, 190)])
    return seqs


def test_reference_is_the_oracle_on_variants_with_n(ca):
    res = orc.pipeline(variant_reads(), do_pass2=False)
    assert len(res.tokens) > 2500 and any(b"N" in t for t in res.tokens)
    assert_reference_is_the_oracle(res)
    for k in (1, 2, 12):                               # the other thresholds, against the host merge (the oracle's list, its tokens)
        chars, lens = ca.dr_slots(res.tokens, stride=64)
        assert_host_merge_is_the_reference(ca.merge_host(chars, lens, k), res.tokens, ms.merge_reference(res.tokens, k))


def assert_host_merge_is_the_reference(m, tokens, ref):
    groups, patterns, pat_group, dropped = ref
    assert m.tokens == list(tokens)
    assert m.cand_token.tolist() == list(range(2, len(tokens) + 2))
    assert m.groups == groups and m.n_groups == len(groups) and m.next_free_gid == len(groups) + 1
    assert m.patterns == patterns
    assert m.pat_group.tolist() == pat_group


@pytest.fixture(scope="module", params=ms.SET_NAMES)
def designed(request):
    return ms.token_set(request.param)


def test_host_merge_is_the_reference(ca, designed):
    ts = designed
    chars, lens = ca.dr_slots(ts.tokens, stride=ts.stride)
    assert_host_merge_is_the_reference(ca.merge_host(chars, lens, ts.k), ts.tokens, ts.reference)
    # the repeats a gathered list holds do not change it: first-occurrence order
    rows = ts.tokens + ts.tokens[::3] + ts.tokens[:2]
    assert ms.dedupe(rows) == ts.tokens
    chars, lens = ca.dr_slots(rows, stride=ts.stride)
    m = ca.merge_host(chars, lens, ts.k)
    assert (m.tokens, m.groups, m.patterns, m.pat_group.tolist()) == (ts.tokens,) + tuple(ts.reference[:3])
    assert m.cand_token.tolist() == [ts.tokens.index(r) + 2 for r in rows]


def test_designed_tokens_have_their_verdict_and_none_is_lost(designed):
    ts = designed
    groups, patterns, pat_group, dropped = ts.reference
    gid = {t - 2: g for g, members in enumerate(groups) for t in members}
    first = {g: members[0] - 2 for g, members in enumerate(groups)}
    assert sorted(t for v in ts.classes.values() for t in v) == sorted(ts.verdict) == list(range(len(ts.tokens)))
    assert all(ms.low_lexi(t) for t in ts.tokens)       # tokens are DRLowLexi forms, as pass 1 makes them: a recruit's DR string is a token
    for cls, members in ts.classes.items():
        assert members, cls
        for t in members:
            v = ts.verdict[t]
            assert v and set(v) <= {"joins", "founds", "dropped"} and not ("joins" in v and "founds" in v)
            if "joins" in v:
                assert v["joins"] < t and gid[t] == gid[v["joins"]] and first[gid[t]] != t, (cls, t, v)
            if "founds" in v:
                assert first[gid[t]] == t, (cls, t)
            if "dropped" in v:
                assert (t in dropped) == v["dropped"], (cls, t)
                assert (ts.tokens[t] in patterns) == (not v["dropped"])
    assert len(patterns) == 2 * (len(ts.tokens) - len(dropped))


def classes_of(name):
    return set(ms.token_set(name).classes)


def test_every_named_class_is_there():
    for k in (1, 2, 6, 12):
        for name in ("cluster-%d" % k, "cluster_wide-%d" % k):
            c = classes_of(name)
            want = {"threshold_%s_%s" % (s, o) for s in ("minus1", "exact", "plus1") for o in ("fwd", "rc")}
            want |= {"chimera_later_group_first", "chimera_earlier_group_first", "addup_brings_kmers", "addup_only_new_kmers", "addup_two_owners",
                     "below_threshold_founds", "joins_the_new_group", "homopolymer_first_holder", "homopolymer_owner", "homopolymer_run13",
                     "homopolymer_run_reaches"}
            if k != 12 or "wide" in name:              # (thr - 1) + thr + 1 sightings in three segments are 2 thr + 30 bases: 54 at k = 12
                want.add("chimera_seen_first_loses")
            want |= {"founder_64", "last_kmers_64", "last_kmers_64_minus1"} if "wide" in name else \
                    {"founder_23", "founder_47", "exact_23_joins", "exact_23_founds", "exact_47_joins", "exact_47_founds"}
            assert want <= c, (name, want - c)
        ts = ms.token_set("cluster-%d" % k)
        assert {23, 47} <= {len(t) for t in ts.tokens} and ts.thr == max(k, 2)
        ts = ms.token_set("cluster_wide-%d" % k)
        assert {len(t) for t in ts.tokens} == {48, 54, 55, 63, 64} and ts.stride == 64
    # at k = 1 a token sharing exactly one 11-mer founds its own group
    ts = ms.token_set("cluster-1")
    for t in ts.classes["threshold_minus1_fwd"] + ts.classes["threshold_minus1_rc"]:
        assert len(ts.sightings(ts.tokens[t])) >= 1 and ts.verdict[t] == {"founds": True}
    c = classes_of("redundant")
    assert {"needle_%s_%s" % (p, o) for p in ("offset0", "middle", "last_offset") for o in ("fwd", "rc")} <= c
    assert {"one_shorter_offset0", "one_shorter_offset1", "equal_length_one_base", "chain_a", "chain_b", "chain_c", "haystack_first",
            "needle_second", "many_needles", "many_needles_haystack", "many_needles_no_needle"} <= c
    assert {"near_miss_%s_%s" % (p, o) for p in ("base17", "last_base") for o in ("fwd", "rc")} <= c
    ts = ms.token_set("redundant")
    assert len(ts.classes["many_needles"]) == 70 and len({ts.tokens[t][:22] for t in ts.classes["many_needles"]}) == 1
    assert {"short_token", "longer_holds_it", "longer_first", "short_second"} <= classes_of("redundant_k20")
    assert ms.token_set("redundant_k20").k == 20 and not ms.token_set("redundant_k20").reference[3]
    c = classes_of("redundant_wide")
    assert {"second_batch_%d" % n for n in range(55, 65)} | {"second_batch_miss_%d" % n for n in range(55, 65)} <= c
    for name, ats in (("n_mask", (30, 35)), ("n_mask_wide", (30, 35, 50, 57))):
        c = classes_of(name)
        for at in ats:
            for o in ("fwd", "rc"):
                assert {"%s_n_at_%d_%s" % (p, at, o) for p in ("n_on_n", "n_needle_a_haystack", "a_needle_n_haystack")} <= c
        assert {"n_kmer_founder", "n_kmers_join_rc", "n_kmers_below_rc", "n_kmers_join_fwd"} <= c
    assert {"n_at_base_63", "a_at_base_63", "n_at_base_63_rc"} <= classes_of("n_mask_wide")
    for k in (2, 6):
        ts = ms.token_set("short_keys-%d" % k)
        assert {"short_token_%d" % n for n in (15, 16, 17, 18)} | {"needle_15", "needle_15_last_offset_16", "needle_15_last_offset_37"} <= set(ts.classes)
        assert (ts.low, ts.high, ts.stride) == (15, 37, 48)
    assert len(ms.token_set("short_keys-2").reference[3]) > 0 and not ms.token_set("short_keys-6").reference[3]
    for name in ("all_t", "t_off8", "all_t_blocked", "all_t_low19"):
        assert len(ms.token_set(name).classes["t_run"]) == 4 and not ms.token_set(name).reference[3]
    assert {"token_22"} <= classes_of("declined_short") and {"token_with_r"} <= classes_of("declined_r")
    lens = sorted(len(t) for t in ms.token_set("declined_short").tokens)
    assert lens[0] == 22 and lens[1] >= 23             # a valid set and ONE token of 22 bases
    assert any(b"R" in t for t in ms.token_set("declined_r").tokens)


def test_all_t_keys():
    """the anchor keys of every pattern (16-mers at offsets 0 .. 7; at lowDRsize 19: at offsets 0 .. 3): all_t holds T*16, twice as a
    pattern's offset 0 and twice as its offset 7 (at lowDRsize 19 only the two at offset 0 are keys); its sister set holds none, and
    A*16 — key 0, the smallest there is — through the reverse complements; every tier set holds T*16 once"""
    for name, at_want in (("all_t", [0, 0, 7, 7]), ("t_off8", []), ("all_t_blocked", [0, 0, 7, 7]), ("all_t_low19", [0, 0]),
                          ("tiers0", [0]), ("tiers1", [0]), ("tiers2", [7])):
        ts = ms.token_set(name)
        pats = ts.reference[1]
        kl, n_off = ms.anchor_shape(ts.low)
        assert (kl, n_off) == ((16, 4) if name == "all_t_low19" else (16, 8))
        at = sorted(r for p in pats for r in range(n_off) if p[r:r + 16] == b"T" * 16)
        assert at == at_want
        keys = ms.anchor_key_strings(pats, ts.low)
        assert (b"T" * 16 in keys) == bool(at_want) and (b"A" * 16 in keys) == (name == "t_off8")
        if ts.low >= 23:
            assert len(keys) == rs.anchor_keys(pats)
    ts = ms.token_set("all_t_low19")
    assert {19, 20, 22} <= {len(t) for t in ts.tokens} and ts.params()["lowDRsize"] == 19
    for k in (2, 6):                                   # 12-base keys at offsets 0 .. 3
        ts = ms.token_set("short_keys-%d" % k)
        assert ms.anchor_shape(ts.low) == (12, 4)
        keys = ms.anchor_key_strings(ts.reference[1], ts.low)
        assert {len(x) for x in keys} == {12} and 0 < len(keys) <= 4 * len(ts.reference[1])


def test_all_t_blocked_takes_both_slots_of_the_all_t_key():
    """the premise of all_t_blocked, for every table size up to 2^12 slots (3 * keys <= 2^log: up to 1 365 keys): both slots of
    T*16 are the first slot of another key; in all_t neither is, at 2^10 slots"""
    pats = ms.token_set("all_t_blocked").reference[1]
    assert len(ms.token_set("all_t_blocked").classes["t_run"]) == 4 and rs.anchor_keys(pats) * 3 <= 1024
    for log in (10, 11, 12):
        assert ms.blocked_slots(pats, log) == [True, True]
    assert ms.blocked_slots(ms.token_set("all_t").reference[1], 10) == [False, False]
    assert ms.ak_hash(0xFFFFFFFF, ms.AK_M[0]) >> 22 != ms.ak_hash(0xFFFFFFFF, ms.AK_M[1]) >> 22


@pytest.mark.parametrize("i", [0, 1, 2])
def test_tiers_land_in_their_key_ranges(i):
    ts = ms.token_set("tiers%d" % i)
    n = rs.anchor_keys(ts.reference[1])
    lo, hi = ms.TIER_KEYS[i]
    assert lo + ms.TIER_MARGIN < n <= hi - ms.TIER_MARGIN
    assert len(ts.reference[0]) == len(ts.tokens) == ms.TIER_TOKENS[i] + 1     # mutually unrelated: every token its own group
    assert len(ts.classes["t_run"]) == 1


@pytest.mark.parametrize("name,layout", ms.READ_CASES, ids=["%s-%s" % c for c in ms.READ_CASES])
def test_designed_reads_have_their_verdict_and_none_is_lost(name, layout):
    c = ms.case(name, layout)
    got = {r[0] for r in rs.find_singletons(c.seqs, c.patterns)}
    assert len(c.designed) + len(c.classes["background"]) == len(c.seqs) and len(c.seqs) % 64 != 0
    for cls, members in c.classes.items():
        assert members, cls
        for i, recruited in members:
            assert (i in got) == recruited, (cls, i, c.seqs[i])
    assert got == c.want() and got
    if name == "redundant_k20":                        # both patterns end at the same base: the longest is reported
        lens = {r[4] for r in rs.find_singletons(c.seqs, c.patterns)}
        assert {25, 37, 45, 47} <= lens
    if ms.token_set(name).run:
        assert {"bare_run_T", "bare_run_A", "bare_k0", "run_in_pattern", "run_one_base_changed"} <= set(c.classes)
    if name.startswith("n_mask"):
        assert {"n_pattern_as_is", "n_pattern_a_for_n", "n_pattern_r_for_n"} <= set(c.classes)


@pytest.mark.parametrize("name,layout", ms.READ_CASES, ids=["%s-%s" % c for c in ms.READ_CASES])
def test_gpu_cases_leave_the_device_merge_no_reason_to_give_up(ca, name, layout):
    """what test_gpu_merge_sets.py's cases rest on, with the oracle's pass 1 in the place of the device's: pass 1 finds head reads
    only and at least one of them, the context's own tokens share no group with the designed ones (every verdict holds on the whole
    list), and the key set has a two-choice placement under the device's hash pair — else the device merge hands over to the host
    merge (a pair of one-slot keys around a third key: t_off8's A*16 makes fourteen one-slot keys), and the GPU case, which
    asserts the device's tables, would be about the host's"""
    from tests.test_gpu_merge_sets import head_reads
    ts, c = ms.token_set(name), ms.case(name, layout)
    seqs = head_reads(ca, ts, layout) + c.seqs
    res = orc.pipeline(seqs, params=orc.Params.default(lowDRsize=ts.low, highDRsize=ts.high, kmer_clust_size=ts.k), do_pass2=False)
    found = {int(r) for r in res.rec_read[:res.n_pass1]}
    assert found and found <= set(range(48)) and res.tokens
    tokens = ms.dedupe(res.tokens + ts.tokens)
    assert tokens[:len(res.tokens)] == res.tokens and len(tokens) == len(res.tokens) + len(ts.tokens)
    groups, patterns, pat_group, dropped = ms.merge_reference(tokens, ts.k)
    gid = {t - 2: g for g, mem in enumerate(groups) for t in mem}
    n_own = len(res.tokens)
    for t, v in ts.verdict.items():
        if "joins" in v:
            assert gid[n_own + t] == gid[n_own + v["joins"]]
        if "dropped" in v:
            assert (ts.tokens[t] in patterns) == (not v["dropped"])
    if not name.startswith("declined"):
        assert not ms.unplaceable_keys(patterns, ts.low)


# ---- the designs reject plausible wrong variants of the clustering rule ----
def cluster_variant(tokens, k, rule):
    """clusterDRReads' group per token with one plausible mistake (rule "right": none)"""
    k2gid, gid, next_gid = {}, [], 1
    for tok in tokens:
        count, homeless, group, seen = {}, [], 0, set()
        thr = k if rule == "first_sighting_compared" else max(k, 2)
        for km in ms.kmers(tok):
            if km not in k2gid:
                homeless.append(km)
                continue
            if rule == "once_per_kmer" and km in seen:
                continue
            seen.add(km)
            g = k2gid[km]
            count[g] = count.get(g, 0) + 1
            if group == 0 and count[g] >= thr:
                group = g
        reached = [g for g in count if count[g] >= thr]
        if rule == "lowest_gid" and reached:
            group = min(reached)
        if rule == "largest_count" and reached:
            group = max(reached, key=lambda g: (count[g], -g))
        if group == 0:
            group = next_gid
            next_gid += 1
        for km in homeless:
            k2gid[km] = group
        gid.append(group)
    return gid


@pytest.mark.parametrize("name", ["cluster-1", "cluster-6", "cluster_wide-12"])
def test_wrong_variants_of_the_clustering_rule_change_a_designed_verdict(name):
    ts = ms.token_set(name)
    right = cluster_variant(ts.tokens, ts.k, "right")
    assert [[t + 2 for t, g in enumerate(right) if g == gg] for gg in range(1, max(right) + 1)] == ts.reference[0]

    def changed(rule):
        wrong = cluster_variant(ts.tokens, ts.k, rule)
        return {cls for cls, members in ts.classes.items() for t in members
                if (wrong[t] == wrong[ts.root(t)]) != (right[t] == right[ts.root(t)]) or
                (wrong[t] in wrong[:t]) != (right[t] in right[:t])}
    if ts.k == 1:                                      # the threshold compared on a first sighting: one shared 11-mer joins
        assert {"threshold_minus1_fwd", "threshold_minus1_rc", "below_threshold_founds"} <= changed("first_sighting_compared")
    else:
        assert not changed("first_sighting_compared")
    assert "chimera_later_group_first" in changed("lowest_gid")
    if "chimera_seen_first_loses" in ts.classes:
        assert "chimera_seen_first_loses" in changed("lowest_gid")
    if ts.k == 6:                                      # (2 thr sightings of the losing group fit the token)
        assert "chimera_later_group_first" in changed("largest_count")
    assert "homopolymer_run_reaches" in changed("once_per_kmer")
