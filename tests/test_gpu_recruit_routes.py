"""Pass 2 on caller-given patterns, the route crass takes through the adapter: crass_hip_load_reads -> crass_hip_set_patterns ->
crass_hip_recruit, without a seed scan (the found flags are cleared when the reads are loaded).  Every case is exact equality
with tests/recruit_sets.find_singletons, field by field and the DR string among them, on designed reads (window edges, near
misses, the first-callback rule, k_recruit_finish's edges, exception reads, the wave scan's slice edges) that
test_recruit_sets_host.py pins on the CPU; and every case asserts the counters that name its route, so that a routing change
cannot move the coverage away quietly.

The routes and where their thresholds come from:

| route                          | condition                                                          | counters                      |
|--------------------------------|--------------------------------------------------------------------|-------------------------------|
| k_recruit<true, 256>           | a pattern under 23 bases (build_anchors gives up); n_states * 10   | used_lds_automaton 1,         |
|                                | bytes <= 40 KB, i.e. ac_states <= 4 096 (launch_recruit_lds)       | ac_states <= 4 096            |
| k_recruit<true, 512>           | 40 KB < n_states * 10 <= 80 KB: ac_states in (4 096, 8 192]        | 1                             |
| k_recruit<true, 1024>          | <= 160 KB: ac_states in (8 192, 16 384]                            | 1                             |
| k_recruit<false, 256>          | ac_states in (16 384, 65 535]                                      | 0                             |
| k_recruit_wide over go32       | ac_states > 65 535 (install_patterns: no 16-bit tables)            | 0                             |
| k_anchor_filter MODE 0         | all patterns >= 23 bases, <= 16 384 distinct keys (build_anchors:  | 2, anchor_table_kind 0        |
|                                | exact keys, 2^15 slots at load <= 1/2)                             |                               |
| MODE 1                         | keys in (16 384, 52 428]: fingerprint buckets, 2^16 slots, <= 0.8  | 2, kind 1                     |
| MODE 2 + k_recruit_list / go4w | keys > 52 428 (log_size > 15: keys in L2) and ac_states > 65 535   | 2, kind 2                     |
| k_recruit_exc + finish<true>   | exception reads beside a MODE 0 set holding a pattern with an N    | 2, n_exceptions > 0           |

ac_states and anchor_keys are also compared with the trie nodes and distinct keys recomputed in Python."""
import os
import random

import numpy as np
import pytest

from tests import recruit_sets as rs

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED, STATE = 0, 1, 2, 6


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


_REF = {}


def reference(key, seqs, patterns, found=(), header_id=None):
    """find_singletons, computed once per key and never changed"""
    if key not in _REF:
        _REF[key] = rs.find_singletons(seqs, patterns, found, header_id)
    return _REF[key]


def run_recruit(ca, seqs, patterns, pad=0, header_id=None, extra_found=None, params=None, env=None, engine=None):
    """SearchEngine(params), load_reads(PackedReads(seqs, pad), header_id), set_patterns(patterns), recruit(extra_found):
    (RecruitSet, counters, (stride_words, uniform_len)).  env: switches set around the context's creation (they are read then).
    engine: a live context whose reads are loaded already — only the patterns are installed."""
    if engine is not None:
        engine.set_patterns(patterns)
        return engine.recruit(extra_found), engine.counters(), None
    os.environ.update(env or {})
    try:
        eng = ca.SearchEngine(params)
    finally:
        for k in env or {}:
            os.environ.pop(k, None)
    packed = ca.PackedReads(seqs, pad)
    try:
        eng.load_reads(packed, header_id)
        layout = (int(packed.reads.stride_words), int(packed.reads.uniform_len))
        eng.set_patterns(patterns)
        return eng.recruit(extra_found), eng.counters(), layout
    finally:
        eng.close()
        packed.close()


def assert_recruits(got, ref, dr_stride=48):
    """exact equality with find_singletons' tuples (read, low_lexi, start, end, dr_len, dr_bytes)"""
    assert got.dr_stride == dr_stride
    assert got.read_idx.tolist() == [r[0] for r in ref]
    assert got.low_lexi.tolist() == [r[1] for r in ref]
    assert got.start.tolist() == [r[2] for r in ref]
    assert got.end.tolist() == [r[3] for r in ref]
    assert got.dr_len.tolist() == [r[4] for r in ref]
    for k, r in enumerate(ref):
        assert got.dr(k) == r[5], (k, r)
        assert int(got.end[k]) - int(got.start[k]) + 1 == int(got.dr_len[k])
        assert not got.dr_chars[k * dr_stride + r[4]:(k + 1) * dr_stride].any()        # the slot is zero behind the string


def assert_route(cnt, name, patterns):
    lds, kind, (s_lo, s_hi), keys = rs.ROUTES[name]
    assert cnt["n_patterns"] == len(patterns)
    assert cnt["used_lds_automaton"] == lds
    assert s_lo < cnt["ac_states"] <= s_hi
    assert cnt["ac_states"] == rs.trie_states(patterns)
    if kind is None:
        assert cnt["anchor_keys"] == 0
    else:
        assert cnt["anchor_table_kind"] == kind
        assert keys[0] < cnt["anchor_keys"] <= keys[1] and cnt["anchor_keys"] == rs.anchor_keys(patterns)


def check_case(ca, name, layout, n_total, pad=0, params=None, env=None, dr_stride=48):
    c = rs.case(name, layout, n_total)
    ref = reference((name, layout, n_total), c.seqs, c.patterns)
    assert {r[0] for r in ref} == c.want() and c.want()                # zero designed reads are left out
    got, cnt, lay = run_recruit(ca, c.seqs, c.patterns, pad=pad, params=params, env=env)
    assert_recruits(got, ref, dr_stride)
    assert_route(cnt, name, c.patterns)
    assert cnt["n_pass2_found"] == len(ref) and cnt["n_reads"] == len(c.seqs)
    return c, cnt, lay


@pytest.mark.parametrize("name,layout,n_total", rs.ROUTE_CASES, ids=[c[0] for c in rs.ROUTE_CASES])
def test_routes(ca, name, layout, n_total):
    """every row of the table above on 2 003 uniform reads of 150 bases (stride 10, the register form W = 10)"""
    c, cnt, lay = check_case(ca, name, layout, n_total)
    assert lay == (10, 150)
    assert cnt["n_exceptions"] == sum(len(c.classes[k]) for k in c.classes if k.startswith("exc_")) > 0
    if name == "npat":
        assert c.classes["exc_n_pattern"] and c.classes["exc_lower_pattern"]


@pytest.mark.parametrize("name,layout,n_total", rs.LAYOUT_CASES, ids=["%s-%s" % c[:2] for c in rs.LAYOUT_CASES])
def test_anchor_probe_layouts(ca, name, layout, n_total):
    """the host-built exact table over every body of the probe: the register form's first and last instantiations and those on
    either side of W = 12 (uniform strides 4 .. 16), a uniform stride of 17 (lane per read), per-read lengths on one stride
    (the vector mask, exception words from the prefetch), the tight ragged layout (four words per round), and the wave walk
    (reads over 800 bases, rounds of 256 windows: h_max 255 | 256 on either side of the first round's end; k_recruit_list_wave
    verifies, over go4 and — mode2 — over go4w)"""
    pad = 2 if layout == "padded" else 0
    c, cnt, lay = check_case(ca, name, layout, n_total, pad=pad)
    if layout[0] == "u":
        L = int(layout[1:])
        assert lay == (rs.UNIFORM_STRIDES[L], L)
    elif layout == "padded":
        assert lay == (10, 0)
    elif layout in ("ragged", "wragged"):
        assert lay == (0, 0)
    else:
        L = int(layout[1:])
        assert lay == ((L + 15) // 16, L)
    if layout[0] == "w":
        assert c.classes["slice_edge"] and c.classes["slice_two_copies"] and max(len(s) for s in c.seqs) > 800
    assert cnt["n_exceptions"] > 0


@pytest.mark.parametrize("name", ["mode0", "lds256"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_read_counts(ca, name, n):
    """one read, and one read less / exactly / one read more than a wave's 64"""
    c = rs.head(rs.case(name, "u150", 2003), n)
    assert len(c.seqs) == n
    ref = reference((name, "head", n), c.seqs, c.patterns)
    assert {r[0] for r in ref} == c.want() and ref
    got, cnt, lay = run_recruit(ca, c.seqs, c.patterns)
    assert_recruits(got, ref)
    assert_route(cnt, name, c.patterns)


@pytest.mark.parametrize("n", [1025, 3073])
def test_probe_as_one_block(ca, n):
    """CRASS_PROBE_BLOCKS=1: the probe is one block of 16 waves, so every wave takes several tiles (1 025 reads: a second,
    one-read tile for wave 0; 3 073: a fourth) — the prefetch chain of the register form over a host-built table"""
    check_case(ca, "mode0", "u150", n, env={"CRASS_PROBE_BLOCKS": "1"})


@pytest.mark.parametrize("name,layout,n_total", rs.WIDE_CASES, ids=[c[1] for c in rs.WIDE_CASES])
def test_long_repeats(ca, name, layout, n_total):
    """highDRsize = 96 (slots of 96 bytes): k_recruit_finish's 128-bit path at 33 .. 64 bases (48, 63, 64: drop < 64 and
    drop == 0) and the byte-wise path beyond (65, 96)"""
    p = ca.default_params(highDRsize=96)
    c, cnt, lay = check_case(ca, name, layout, n_total, params=p, dr_stride=96)
    lens = {r[4] for r in reference((name, layout, n_total), c.seqs, c.patterns)}
    assert {23, 31, 32, 33, 47, 48, 63, 64, 65, 96} <= lens


def test_exception_reads_on_a_padded_stride(ca):
    """the set with an N pattern on per-read lengths: the probe skips exception reads by the prefetched exception word, the byte
    automaton recruits them"""
    c, cnt, lay = check_case(ca, "npat", "padded", 2003, pad=2)
    assert lay == (10, 0) and cnt["n_exceptions"] > 0 and c.classes["exc_n_pattern"]


def test_extra_found_and_header_ids(ca):
    """found headers of other shards (launch_mark_found): a third of the recruitable reads are listed and vanish, together
    with the reads sharing their header id; an index beyond the read set is an invalid argument"""
    c = rs.case("mode0", "u150", 2003)
    want = sorted(c.want())
    hid = np.arange(len(c.seqs), dtype=np.uint64)
    for a, b in zip(want[0::4], want[1::4]):           # every fourth recruitable read shares its header with the next one
        hid[b] = a
    extra = want[0::3]
    ref = reference("extra_found", c.seqs, c.patterns, extra, hid)
    plain = reference("header ids only", c.seqs, c.patterns, (), hid)
    assert len(plain) == len(want) and len(ref) < len(want) - len(extra), "reads must vanish for their header id alone"
    got, cnt, lay = run_recruit(ca, c.seqs, c.patterns, header_id=hid, extra_found=extra)
    assert_recruits(got, ref)
    got, cnt, lay = run_recruit(ca, c.seqs, c.patterns, header_id=hid)
    assert_recruits(got, plain)
    with pytest.raises(ca.CrassError) as e:
        run_recruit(ca, c.seqs, c.patterns, header_id=hid, extra_found=[want[0], len(c.seqs)])
    assert e.value.status == INVALID_ARG


def test_pattern_sets_in_turn_on_one_context(ca):
    """go32, MODE 0, 256-thread LDS, the empty list, MODE 2 installed one after the other on a live context: each result is the
    reference's and a fresh context's — nothing of the set before (tables, anchors, go16 / go32) survives"""
    names = ["go32", "mode0", "lds256", None, "mode2"]
    seqs = [s for nm in names if nm for s in rs.case(nm, "u150", 2003).seqs]
    assert len(seqs) % 64 != 0
    eng = ca.SearchEngine()
    packed = ca.PackedReads(seqs, 0)
    try:
        eng.load_reads(packed)
        for nm in names:
            pats = rs.pattern_set(nm)[0] if nm else []
            ref = reference(("in turn", nm), seqs, pats)
            got, cnt, _ = run_recruit(ca, seqs, pats, engine=eng)
            assert_recruits(got, ref)
            fresh, fcnt, _ = run_recruit(ca, seqs, pats)
            assert_recruits(fresh, ref)
            if nm:
                assert len(ref) > 200
                assert_route(cnt, nm, pats)
                for k in ("used_lds_automaton", "anchor_table_kind", "anchor_keys", "ac_states", "n_patterns", "n_pass2_found"):
                    assert cnt[k] == fcnt[k], k
            else:
                assert got.n == 0 and cnt["n_patterns"] == 0 and cnt["ac_states"] == 0
    finally:
        eng.close()
        packed.close()


def test_status_codes(ca):
    """a zero-length pattern, a 256-base pattern and a pattern longer than the recruit slot (49 bases under the default
    highDRsize of 47: dr_stride 48) are declined as a whole set, the context then has no patterns; the same 49 bases under
    highDRsize = 96 are accepted and recruited; a valid set installed afterwards recruits correctly"""
    c = rs.case("mode0_small", "u150", 2003)
    ref = reference(("mode0_small", "u150", 2003), c.seqs, c.patterns)
    p49 = rs._rand(random.Random(49), 49)
    seqs = list(c.seqs) + [rs._place(random.Random(50), 150, o, p49) for o in (0, 5, 101)]
    packed = ca.PackedReads(seqs, 0)
    try:
        for params, stride in ((None, 48), (ca.default_params(highDRsize=96), 96)):
            eng = ca.SearchEngine(params)
            try:
                eng.load_reads(packed)
                eng.set_patterns(c.patterns)
                assert_recruits(eng.recruit(), ref, stride)
                bad_sets = [c.patterns + [b""], c.patterns + [b"A" * 256]] + ([c.patterns + [p49]] if stride == 48 else [])
                for bad in bad_sets:
                    with pytest.raises(ca.CrassError) as e:
                        eng.set_patterns(bad)
                    assert e.value.status == UNSUPPORTED
                    with pytest.raises(ca.CrassError) as e:
                        eng.recruit()
                    assert e.value.status == STATE
                pats = c.patterns + ([p49] if stride == 96 else [])
                eng.set_patterns(pats)
                want = rs.find_singletons(seqs, pats)
                assert len(want) == len(ref) + (3 if stride == 96 else 0)
                assert_recruits(eng.recruit(), want, stride)
            finally:
                eng.close()
    finally:
        packed.close()
