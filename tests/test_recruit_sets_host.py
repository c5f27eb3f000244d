"""tests/recruit_sets.py pinned on the CPU, before test_gpu_recruit_routes.py trusts it: the reference find_singletons against
the oracle's own pass 2 (whole pipeline, found reads and duplicate headers among them), against a brute-force first match and,
where oracle/_ref exists, against the compiled reference's matcher; every designed class non-empty and with the verdict it
was designed for; every pattern set in the tier its route claims; and three plausible wrong variants of the rule, each of
which changes the record of at least one designed read."""
import os

import numpy as np
import pytest

from tests import orc, fastx
from tests import recruit_sets as rs

DATA = os.path.join(os.path.dirname(__file__), "golden", "data")


def header_ids(hdrs):
    first = {}
    return [first.setdefault(h, i) for i, h in enumerate(hdrs)]


def oracle_pass2(res):
    n1, n = res.n_pass1, res.n_pass1 + res.n_pass2
    out = []
    for k in range(n1, n):
        ss = res.ss(k)
        assert len(ss) == 2
        out.append((int(res.rec_read[k]), int(res.rec_lowlexi[k]), ss[0], ss[1]))
    return out


def check_against_pipeline(seqs, hdrs):
    res = orc.pipeline(seqs, hdrs)
    assert res.error == 0 and res.n_pass1 > 0 and res.n_pass2 > 0
    found = [int(r) for r in res.rec_read[:res.n_pass1]]
    got = rs.find_singletons(seqs, [bytes(p) for p in res.patterns], found, header_ids(hdrs) if hdrs else None)
    assert [g[:4] for g in got] == oracle_pass2(res)
    for j, (r, low, start, end, dl, dr) in enumerate(got):
        assert end - start + 1 == dl == len(dr)
        assert res.tokens[int(res.rec_token[res.n_pass1 + j]) - 2] == dr       # addReadHolder's token is the DR string
    return res, got


@pytest.mark.parametrize("fname", ["Ill.nr.miss.fa.gz", "front_offset_bug.fa.gz"])
def test_reference_reproduces_the_oracles_pass2_on_golden_files(fname):
    recs = fastx.read_fastx(os.path.join(DATA, fname))
    check_against_pipeline([r[2] for r in recs], [r[0] for r in recs])


def test_reference_reproduces_the_oracles_pass2_with_duplicate_headers():
    """a synthetic set (the generator of the GPU tests, which runs on the host) whose headers repeat: a read sharing its header
    with a read pass 1 found is not recruited, and the reference must drop it by header id"""
    import random
    import crass_amd as ca
    spec = ca.synth_spec(read_len=150, crispr_per_million=150000)
    n = 3000
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), 10, 150, n)
    seqs = [asc[i * 150:(i + 1) * 150].tobytes() for i in range(n)]
    rng = random.Random(3)
    hdrs = [b"r%d" % (i if rng.random() > 0.2 else rng.randrange(0, i + 1)) for i in range(n)]
    res, got = check_against_pipeline(seqs, hdrs)
    plain = rs.find_singletons(seqs, [bytes(p) for p in res.patterns], [int(r) for r in res.rec_read[:res.n_pass1]])
    assert len(plain) > len(got), "no read was dropped for its header alone: the set does not test header ids"
    check_against_pipeline(seqs, None)


@pytest.fixture(scope="module", params=rs.ALL_CASES, ids=lambda c: "%s-%s-%d" % c)
def built(request):
    c = rs.case(*request.param)
    return request.param, c, rs.find_singletons(c.seqs, c.patterns)


def test_designed_reads_have_their_verdict_and_none_is_lost(built):
    (name, layout, n_total), c, ref = built
    got = {r[0] for r in ref}
    assert len(c.seqs) >= n_total and len(c.designed) + len(c.classes["background"]) == len(c.seqs)
    for cls, members in c.classes.items():
        assert members, cls
        for i, recruited in members:
            assert (i in got) == recruited, (cls, i, c.seqs[i])
    assert not any(i in got for i, _ in c.classes["background"])
    assert len(got) == len(c.want())                   # every designed recruit is kept, and nothing else is recruited
    assert len(c.seqs) % 64 != 0
    for r, low, start, end, dl, dr in ref:
        assert end - start + 1 == dl == len(dr) and 0 <= start <= end < len(c.seqs[r])


def test_reference_is_the_brute_force_first_match(built):
    (name, layout, n_total), c, ref = built
    by_read = {r[0]: r for r in ref}
    sm = rs.SliceMatcher(c.patterns)
    for i in range(len(c.seqs)):
        m = sm.first(c.seqs[i])
        assert (m is None) == (i not in by_read), i
        if m:
            assert by_read[i] == rs.record(i, c.seqs[i], *m)
    # bytes.find over every pattern: all designed reads of the small sets, two of each class of the large ones
    if len(c.patterns) <= 400:
        pick = [i for i, _ in c.designed]
    else:
        pick = [i for k, v in c.classes.items() for i, _ in v[:2]]
    for i in pick:
        m = rs.brute_first(c.seqs[i], c.patterns)
        assert (m is None) == (i not in by_read), i
        if m:
            assert by_read[i] == rs.record(i, c.seqs[i], *m)


def test_reference_is_the_compiled_matcher(built):
    if orc.ref() is None:
        pytest.skip("oracle/_ref is not built here")
    (name, layout, n_total), c, ref = built
    by_read = {r[0]: r for r in ref}
    ps = orc.PatternSet(list(c.patterns), "ref")
    for i, s in enumerate(c.seqs):
        m = ps.first(s)
        assert (m is None) == (i not in by_read), i
        if m:
            assert by_read[i] == rs.record(i, s, *m)
    ps.close()


@pytest.mark.parametrize("name", sorted(rs.ROUTES))
def test_pattern_sets_fall_into_their_tiers(name):
    """states = trie nodes (root included), keys = distinct 16-mers at offsets 0 .. 7 of the pure-ACGT patterns; the thresholds
    are launch_recruit_lds' (n_states * 10 bytes against 40 / 80 / 160 KB), install_patterns' (65 535 states) and build_anchors'
    (16 384 keys exact in LDS, 52 428 in fingerprint buckets, any ACGT pattern under 23 bases: no anchors)"""
    pats, core = rs.pattern_set(name)
    lds, kind, (s_lo, s_hi), keys = rs.ROUTES[name]
    assert all(p in pats for p in core.values())
    assert s_lo < rs.trie_states(pats) <= s_hi
    nk = rs.anchor_keys(pats)
    if keys is None:
        assert nk is None and min(len(p) for p in pats) == 20
    else:
        assert nk is not None and keys[0] < nk <= keys[1]
        assert all(len(p) >= 23 for p in pats)
    assert max(len(p) for p in pats) <= (96 if name == "mode0_wide" else 47)
    if name == "npat":
        assert rs.N_PATTERN in pats and rs.LOWER_PATTERN in pats


def test_layouts_are_the_ones_the_routes_need():
    """the packers' layout decision for each read layout (crass_pack_layout runs on the host)"""
    import crass_amd as ca

    def lay(layout, n, pad):
        c = rs.case("mode0", layout, n)
        off = np.zeros(len(c.seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in c.seqs])
        return ca.pack_layout(off, pad)
    for L, W in rs.UNIFORM_STRIDES.items():
        assert lay("u%d" % L, 2003, 0) == (W, L)
    assert lay("padded", 2003, 2) == (10, 0)
    assert lay("ragged", 2003, 0) == (0, 0)
    for L in rs.WAVE_LENGTHS:
        assert lay("w%d" % L, 300, 0) == ((L + 15) // 16, L) and L > 800
        assert ((L - 16) >> 3) in (98, 254, 255, 256)
    assert lay("wragged", 700, 0) == (0, 0)
    c = rs.case("mode0", "ragged", 2003)
    assert {1, 15, 16, 22, 23} <= {len(s) for s in c.seqs}


# ---- the reference rejects plausible wrong variants of the rule ----
def designed_records(c, first, **kw):
    out = {}
    for i, _ in c.designed:
        m = first(c.seqs[i])
        if m:
            out[i] = rs.record(i, c.seqs[i], m[0], m[1], **kw)
    return out


def test_wrong_variants_of_the_rule_change_a_designed_record():
    c = rs.case("mode0_small", "u150", 2003)
    ref = {r[0]: r for r in rs.find_singletons(c.seqs, c.patterns)}
    right = designed_records(c, lambda s: rs.brute_first(s, c.patterns))
    assert right == {i: ref[i] for i in right} and len(right) == len(c.want())
    # the shortest pattern reported on ties
    wrong = designed_records(c, lambda s: rs.brute_first(s, c.patterns, tie="shortest"))
    diff = [i for i in right if wrong[i] != right[i]]
    assert {i for i, _ in c.classes["first_callback_suffix"]} <= set(diff)
    assert all(right[i][4] == 40 and wrong[i][4] == 25 for i in diff)      # "long" and its proper suffix end at the same base
    # <= for < in the low-lexi choice: only a repeat equal to its reverse complement can tell
    wrong = designed_records(c, lambda s: rs.brute_first(s, c.patterns), less=lambda a, b: a <= b)
    diff = [i for i in right if wrong[i] != right[i]]
    palin = rs.core_patterns()["palin"]
    assert {i for i, _ in c.classes["palindrome"]} <= set(diff) and all(right[i][5] == palin for i in diff)
    # the end taken inclusive
    wrong = designed_records(c, lambda s: rs.brute_first(s, c.patterns), end_inclusive=True)
    diff = [i for i in right if wrong[i] != right[i]]
    assert len(diff) > len(right) // 2                 # (a copy ending at the read's last base is clamped back: no difference)
