"""The device merge (dmerge.hip) and the pass-2 tables it builds, on the designed token sets of tests/merge_sets.py.  The way in is
crass_hip_merge_distinct: caller-given rows are uploaded, de-duplicated on the device (first-occurrence order) and merged on the
device; a few synthetic CRISPR reads in front of the designed reads leave pass 1 a device-resident distinct list, without which
the device merge does not apply.  The rows are the context's own distinct strings, the designed tokens and a few repeats of
earlier rows.  Every case is exact equality with merge_reference(dedupe(rows), k) — tokens, groups, the pattern list with its
order, pattern groups, next_free_gid, the candidates' tokens — and, for pass 2 over the tables the device built from them, with
recruit_sets.find_singletons over the reference's patterns, field by field.  test_merge_sets_host.py pins the sets, the verdict of
every designed token and read, and the reference itself on the CPU.

The kernels of dmerge.hip and the designed classes (merge_sets.py) that reach their branches:

| kernel                | branch                                                    | designed class                                      |
|-----------------------|-----------------------------------------------------------|-----------------------------------------------------|
| k_dm_init             | tables sized for the token count                          | every set (10 .. 3 400 tokens)                      |
| k_dm_pack_codes       | bases 47 .. 63 of the planes, 54 11-mers                  | cluster_wide: founder_64, last_kmers_64             |
|                       | an N: mask bit, 11-mer identity from the string table     | n_mask: n_kmers_join_rc / _below_rc / _join_fwd     |
|                       | a token under lowDRsize, a base outside ACGTN: fail bit 1 | declined_short, declined_r                          |
| k_dm_greedy           | thr = max(k, 2): a single shared 11-mer does not join     | cluster-1: threshold_minus1_*                       |
|                       | thr - 1 | thr | thr + 1 sightings, through the rev. compl. | cluster, cluster_wide, short_keys: threshold_*      |
|                       | the first group to reach thr along the token wins         | chimera_later_group_first, _earlier_group_first,    |
|                       |                                                           | chimera_seen_first_loses                            |
|                       | prefix count per root, across owner tokens                | addup_*, below_threshold_founds, joins_the_new_group|
|                       | one count per occurrence; o == t is no sighting           | homopolymer_run13, _run_reaches, _first_holder      |
|                       | the needle key cut to 15 bases                            | short_keys: short_token_15, needle_15               |
| k_dm_rd_bases / _fill | > 64 members under one key                                | redundant: many_needles                             |
| k_dm_redundant        | first / last window, both orientations                    | needle_offset0_*, needle_middle_*, needle_last_*    |
|                       | leni < lenj, leni == lenj - 1, equal lengths              | one_shorter_*, equal_length_one_base                |
|                       | the key matches, the comparison fails                     | near_miss_base17_*, near_miss_last_base_*           |
|                       | second round of 64 windows (tokens >= 55 bases)           | redundant_wide: second_batch_55 .. 64, _miss_*      |
|                       | second round of 64 candidates                             | many_needles_haystack, many_needles_no_needle       |
|                       | N against A through mf and the reversed mask mr           | n_mask: n_on_n_*, n_needle_a_haystack_*,            |
|                       |                                                           | a_needle_n_haystack_*, n_at_base_63(_rc)            |
|                       | members of other groups are no needles                    | redundant_k20                                       |
| k_dm_keys             | the key 0xFFFFFFFF: all_t                                 | all_t (t_off8: the same tokens without such a key)  |
|                       | 12-base keys at offsets 0 .. 3 (anchor_keys asserted)     | short_keys                                          |
|                       | 16-base keys at offsets 0 .. 3, T*16 among them           | all_t_low19 (lowDRsize 19)                          |
| k_dm_key_bases_insert | the three tiers of dm_table_params; cuckoo insertion      | tiers0 / tiers1 / tiers2                            |
|                       | the all-T key is not inserted: found through a free slot  | all_t                                               |
|                       | ... its first slot is kept free of other keys             | all_t_blocked (keys whose first slot is either of   |
|                       |                                                           | the all-T key's two slots)                          |
| k_dm_fill_finish      | free slots filled with k0, or left when all_t             | t_off8 (k0 = 0: bare_run_A reads), all_t (bare_run_T)|
|                       | all_t with tab_mode 3 (v = 0xFFFFFFFF), with the Bloom    | tiers1 / tiers2: t_run (one T*16 key per tier set)  |
|                       | filter of the tables probed in L2                         |                                                     |
|                       | plane 2 of the entries (bases 32 .. 63, N mask)           | cluster_wide, redundant_wide, n_mask_wide reads     |
|                       | tab_mode 3: the other slot per key                        | tiers1                                              |
| k_dmx_count / _tiles  | several tiles of 1 024 tokens                             | tiers1, tiers2 under CRASS_DEVICE_VIEW=1            |
| k_dmx_apply / _place  | GIDs in root order, token strings of 15 .. 64 bases       | every set under CRASS_DEVICE_VIEW=1                 |
| k_dmx_sort            | a group of 65 .. view_sort_max members                    | redundant (a group of 78) under CRASS_DEVICE_VIEW=1 |
| k_dmx_rank            | the same group by counting                                | redundant under CRASS_VIEW_SORT_MAX=64              |
| k_dm_verify           | three reads per wave | one read per wave, words in LDS |   | layouts u150 | u184, u304 | u320 | ragged           |
|                       | global loads beyond DV_MAXW | per-read lengths            |                                                     |
|   dv_candidates       | ties: the longest pattern                                 | redundant_k20 reads                                 |
|                       | N in the pattern against N, A, R in the read              | n_mask reads: n_pattern_as_is / _a_for_n / _r_for_n |
|                       | > 64 entries under one key                                | redundant: many_needles reads (70 patterns, one key)|
(k_xg_fill / k_xg_unpack belong to the exchange of a group and are covered by the group tests.)"""
import os

import pytest

from tests import merge_sets as ms
from tests import recruit_sets as rs
from tests.test_gpu_parity import synth_reads
from tests.test_gpu_recruit_routes import assert_recruits

pytestmark = pytest.mark.gpu

ENVS = {
    "default": {},
    "device_view": {"CRASS_DEVICE_VIEW": "1"},
    "device_view_sort64": {"CRASS_DEVICE_VIEW": "1", "CRASS_VIEW_SORT_MAX": "64"},
    "host_merge": {"CRASS_HOST_MERGE": "1"},
}
DECLINED = ("declined_short", "declined_r")
TIER_KIND = {"tiers0": 0, "tiers1": 1, "tiers2": 2}    # anchor_table_kind: exact keys in LDS | 2^16 slots, 16 bits each in LDS | probed in L2


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


_HEADS, _REF = {}, {}
HEAD_FIRST = 0        # the first synthetic read of the head reads (test_merge_sets_host.py: every case's key set has a placement)


def head_reads(ca, ts, layout):
    """a handful of synthetic CRISPR reads of the layout's length: pass 1 finds them and leaves its distinct list on the device"""
    L = 150 if layout == "ragged" else int(layout[1:])
    key = (L, ts.low, ts.high)
    if key not in _HEADS:
        kw = dict(dr_len_min=24, dr_len_max=min(32, ts.high)) if ts.high < 47 else {}
        _HEADS[key] = synth_reads(ca, 48, first=HEAD_FIRST, read_len=L, n_dr=3, crispr_per_million=700000, **kw)
    return _HEADS[key]


def new_engine(ca, ts, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ca.SearchEngine(ca.default_params(**ts.params()))       # (the switches are read when the context is created)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def reference(key, tokens, k, seqs, found):
    """merge_reference and find_singletons over its patterns, computed once per key and never changed"""
    if key not in _REF:
        m = ms.merge_reference(tokens, k)
        _REF[key] = (tokens, m, rs.find_singletons(seqs, m[1], found))
    assert _REF[key][0] == tokens                      # pass 1's part of the rows is the same in every run
    return _REF[key][1], _REF[key][2]


def step(ca, eng, name, layout, keep):
    """load the case's reads behind the head reads, seed scan, merge_distinct over own rows + designed tokens + repeats, recruit:
    every field against the references; returns (case, counters, merge view, reference recruits).  keep: the packed reads, for the
    caller to close behind the context"""
    ts, c = ms.token_set(name), ms.case(name, layout)
    seqs = head_reads(ca, ts, layout) + c.seqs
    packed = ca.PackedReads(seqs, 0)
    keep.append(packed)
    eng.load_reads(packed)
    cand = eng.seed_scan()
    chars, lens, cmap = eng.distinct()
    own = [chars[i, :lens[i]].tobytes() for i in range(len(lens))]
    assert own and len(cmap) == cand.n and chars.shape[1] == ts.stride
    rows = own + ts.tokens + own[:2] + ts.tokens[::5] + own[-1:]        # (the repeats: the device's first-occurrence order)
    tokens = ms.dedupe(rows)
    assert len(tokens) < len(rows) and tokens[:len(own)] == own
    g_chars, g_lens = ca.dr_slots(rows, stride=ts.stride)
    eng.merge_distinct(g_chars, g_lens, 0, fetch=False)
    got = eng.recruit()
    m = eng.merge_view()
    cnt = eng.counters()
    found = sorted({int(r) for r in cand.read_idx})
    assert found
    (groups, patterns, pat_group, dropped), ref = reference((name, layout), tokens, ts.k, seqs, found)
    assert m.tokens == tokens
    assert m.groups == groups and m.n_groups == len(groups) and m.next_free_gid == len(groups) + 1
    assert m.patterns == patterns
    assert m.pat_group.tolist() == pat_group
    assert m.cand_token.tolist() == [tokens.index(cand.dr(k)) + 2 for k in range(cand.n)] == [int(x) + 2 for x in cmap]
    # the designed part of the view, by the designed verdicts (test_merge_sets_host.py: they are the reference's on the set alone,
    # and the context's own tokens share no group with them)
    gid = {t - 2: g for g, mem in enumerate(m.groups) for t in mem}
    for t, v in ts.verdict.items():
        if "joins" in v:
            assert gid[len(own) + t] == gid[len(own) + v["joins"]], (name, t, v)
        if "dropped" in v:
            assert (ts.tokens[t] in m.patterns) == (not v["dropped"]), (name, t, v)
    # pass 2 over the tables built from this merge
    assert set(found) <= set(range(48))                 # pass 1 finds head reads only: every designed read is pass 2's
    want = {i + 48 for i in c.want()}
    assert {r[0] for r in ref if r[0] >= 48} == want and want           # zero designed reads are left out
    assert_recruits(got, ref, ts.stride)
    assert [m.tokens[int(t) - 2] for t in got.token] == [r[5] for r in ref]         # addReadHolder: the DR string's token
    assert cnt["n_pass2_found"] == len(ref) and cnt["n_reads"] == len(seqs) and cnt["n_patterns"] == len(patterns)
    return c, cnt, m, ref


def check_route(name, env, cnt, m):
    if env == "host_merge":
        assert cnt["used_device_merge"] == 0 and cnt["n_merge_fallbacks"] == 0
        return
    if name in DECLINED:
        assert cnt["used_device_merge"] == 0 and cnt["n_merge_fallbacks"] >= 1 and cnt["last_fallback_bits"] & 1
        return
    assert cnt["used_device_merge"] == 1 and cnt["n_merge_fallbacks"] == 0
    assert cnt["used_lds_automaton"] == 2              # anchor probe + k_dm_verify over the device-built tables
    if env.startswith("device_view"):
        assert cnt["used_device_view"] == 1 and cnt["n_view_fallbacks"] == 0
    # the distinct keys k_dm_keys claimed: 16-mers at offsets 0 .. 7, at lowDRsize 19 .. 22 at offsets 0 .. 3, at 15 .. 18 12-mers there
    assert cnt["anchor_keys"] == len(ms.anchor_key_strings(m.patterns, ms.token_set(name).low))
    if name in TIER_KIND:
        assert cnt["anchor_table_kind"] == TIER_KIND[name]
        lo, hi = ms.TIER_KEYS[TIER_KIND[name]]
        assert lo < cnt["anchor_keys"] <= hi
    else:
        assert cnt["anchor_table_kind"] == 0


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("name", ms.SET_NAMES)
def test_designed_sets(ca, name, env):
    """every set on 2 003 reads of 150 bases, under the default switches, with the view assembled on the device (the group of 78
    members on either side of the sort range) and with the host merge: the same view and the same recruits every time"""
    eng, keep = new_engine(ca, ms.token_set(name), ENVS[env]), []
    try:
        c, cnt, m, ref = step(ca, eng, name, "u150", keep)
    finally:
        eng.close()
        for p in keep:
            p.close()
    check_route(name, env, cnt, m)
    if name == "redundant":
        assert max(len(g) for g in m.groups) == 78                       # beyond 64: k_dmx_sort, or k_dmx_rank by counting
    if name == "redundant_k20":
        assert {25, 37, 45, 47} <= {r[4] for r in ref}                 # ties: the longest pattern, through the device's tables
    if name == "all_t_blocked" and env != "host_merge":
        log = min(x for x in (10, 11, 12) if cnt["anchor_keys"] * 3 <= 1 << x)           # dm_table_params
        assert ms.blocked_slots(m.patterns, log) == [True, True]                         # the set's premise
    if ms.token_set(name).run:                         # the all-T sets and the tier sets (one T*16 key in each table form)
        rec = {r[0] - 48 for r in ref}
        assert {i for i, _ in c.classes["run_in_pattern"]} <= rec
        assert not rec & {i for k in ("bare_run_T", "bare_run_A", "bare_k0", "run_one_base_changed") for i, _ in c.classes[k]}
    if name.startswith("n_mask"):
        rec = {r[0] - 48 for r in ref}
        assert {i for i, _ in c.classes["n_pattern_as_is"]} <= rec
        assert not rec & {i for k in ("n_pattern_a_for_n", "n_pattern_r_for_n") for i, _ in c.classes[k]}


LAYOUT_CASES = [c for c in ms.READ_CASES if c[1] != "u150"]


@pytest.mark.parametrize("name,layout", LAYOUT_CASES, ids=["%s-%s" % c for c in LAYOUT_CASES])
def test_verify_layouts(ca, name, layout):
    """k_dm_verify's other forms over the device-built index: one read per wave with the words staged in LDS (184 and 304 bases),
    global loads beyond DV_MAXW words (320 bases), per-read lengths (ragged)"""
    eng, keep = new_engine(ca, ms.token_set(name), {}), []
    try:
        c, cnt, m, ref = step(ca, eng, name, layout, keep)
    finally:
        eng.close()
        for p in keep:
            p.close()
    check_route(name, "default", cnt, m)


@pytest.mark.parametrize("env", ["default", "device_view"])
def test_sets_in_turn_on_one_context(ca, env):
    """a second and a third step on a live context (the seed scan queues a merge of the context's own tokens ahead of the call;
    merge_distinct replaces it): nothing of the set before survives — tokens, groups, tables, the all-T flag"""
    eng, keep = new_engine(ca, ms.token_set("all_t"), ENVS[env]), []
    try:
        for name in ("all_t", "redundant", "t_off8", "tiers1", "cluster-6"):
            c, cnt, m, ref = step(ca, eng, name, "u150", keep)
            check_route(name, env, cnt, m)
    finally:
        eng.close()
        for p in keep:
            p.close()
