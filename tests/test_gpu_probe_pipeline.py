"""Pass 2's anchor probe (pass2.hip, anchor_filter_body<W > 0>) as a software pipeline: a tile's rows, found flags, lengths and
exception words are requested one tile ahead, its header ids two tiles ahead, and a uniform read's windows behind its end are
not probed.  With CRASS_PROBE_BLOCKS=1 the probe is ONE block of 16 waves, so a few thousand reads are several tiles per wave:
first and last turns of the prefetch chain, tiles that end inside a wave, waves whose chain ends early.  Every case is the whole
pipeline against the oracle, record by record."""
import os
import random

import pytest

from tests import orc
from tests.parity import assert_same_pipeline
from tests.test_gpu_parity import synth_reads, to_orc_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


def run_one_block(ca, seqs, hdrs=None, env=None, **kw):
    """search_pipeline (a context of its own: the switches are read when it is created) with the probe capped to one block"""
    env = dict(env or {}, CRASS_PROBE_BLOCKS="1")
    os.environ.update(env)
    try:
        return ca.search_pipeline(seqs, hdrs, **kw)
    finally:
        for k in env:
            os.environ.pop(k, None)


_BASE = {}


def base_set(ca):
    """3 073 uniform reads of 150 bases and the oracle's answer for them (computed once, never changed)"""
    if not _BASE:
        seqs = synth_reads(ca, 3073, read_len=150, crispr_per_million=150000)
        _BASE["seqs"], _BASE["ref"] = seqs, orc.pipeline(seqs)
    return _BASE["seqs"], _BASE["ref"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 3073])
def test_tile_edges(ca, n):
    """One block of 16 waves: 1 024 reads are one tile per wave, 1 025 a second, one-read tile for wave 0, 3 073 a fourth one-read
    tile for wave 0 while every other wave's chain of requests ends one and two tiles before the end; 1 .. 65 reads leave most
    waves without any tile.  The first n reads of a set would hold no read for pass 2 to recruit at the small counts, so the
    n reads are chosen from the 3 073: reads pass 1 finds and reads pass 2 recruits first, in turn, then the rest in order.
    (One read cannot be recruited — a pattern needs a read pass 1 found, and that read is found: n = 1 checks parity only.)"""
    seqs, ref = base_set(ca)
    assert ref.n_pass1 > 0 and ref.n_pass2 > 0
    if n == len(seqs):
        sub = seqs
    else:
        p1 = [int(r) for r in ref.rec_read[:ref.n_pass1]]
        p2 = [int(r) for r in ref.rec_read[ref.n_pass1:ref.n_pass1 + ref.n_pass2]]
        order, seen = [], set()
        for k in range(max(len(p1), len(p2))):
            for lst in (p1, p2):
                if k < len(lst) and lst[k] not in seen:
                    seen.add(lst[k]); order.append(lst[k])
        order += [i for i in range(len(seqs)) if i not in seen]
        sub = [seqs[i] for i in order[:n]]
    gpu = run_one_block(ca, sub)
    assert_same_pipeline(gpu, ref if n == len(seqs) else orc.pipeline(sub))
    if n > 1:
        assert gpu.n_pass2 > 0
    assert gpu.counters["used_device_merge"] == 1


def _filler(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


@pytest.mark.parametrize("L", [144, 145, 151, 152, 159, 160, 161])
def test_last_windows_of_a_uniform_read(ca, L):
    """Strides of 9, 10 and 11 words, every position of the read's end inside its last word pair.  A pattern occurring at offset o
    is seen by ONE window, the aligned one at ceil8(o); the windows behind the read's last one are no longer probed.  Designed
    reads, random but for one copy of a repeat pass 1 found in the same set: the copy ending at the read's last base and 1 .. 8
    bases before it (so its window is the read's last one, or the one before) — recruited —, and the copy with its last base cut
    off at the read's end — not recruited, unless the oracle says otherwise."""
    rng = random.Random(L)
    base = synth_reads(ca, 3000, read_len=L, crispr_per_million=150000, dr_len_min=23, dr_len_max=27)
    ref0 = orc.pipeline(base, do_pass2=False)         # pass 1 and the merge: its tokens and the pattern set
    pats = [bytes(p) for p in ref0.patterns]
    toks = sorted({bytes(t) for t in ref0.tokens if bytes(t) in pats}, key=lambda t: (len(t), t))
    assert toks and len(toks[0]) <= 24, "the set must hold short repeats: only they can sit in the last window"
    picked = toks[:6] + toks[-2:]
    seqs, want, cut = list(base), [], []
    for t in picked:
        for back in range(0, 9):                      # the copy ends `back` bases before the read's end
            s = _filler(rng, L - len(t) - back) + t + _filler(rng, back)
            want.append(len(seqs)); seqs.append(s)
        s = _filler(rng, L - len(t) + 1) + t[:-1]     # the last base does not fit
        if not any(p in s for p in pats):
            cut.append(len(seqs)); seqs.append(s)
    assert cut
    ref = orc.pipeline(seqs)
    recruited = set(int(r) for r in ref.rec_read[ref.n_pass1:ref.n_pass1 + ref.n_pass2])
    assert all(i in recruited for i in want) and not any(i in recruited for i in cut)
    gpu = run_one_block(ca, seqs)
    assert_same_pipeline(gpu, ref)
    got = set(int(r) for r in gpu.rec_read[gpu.n_pass1:gpu.n_pass1 + gpu.n_pass2])
    assert all(i in got for i in want) and not any(i in got for i in cut)


def designed_copies(ca, L, n_base, offsets, kw=None, synth_kw=None):
    """The construction of test_last_windows_of_a_uniform_read for any read length and option set, the probe at its default grid:
    a synthetic base set, then designed reads — random but for one copy of a repeat pass 1 found in the base set, at every
    offset offsets(L, len(repeat)) gives (recruited), and one with the copy's last base cut off at the read's end (not
    recruited).  The whole pipeline against the oracle, and the preconditions of the existing test: `want` all recruited by the
    oracle, `cut` none, the table built on the device."""
    kw = kw or {}
    low = kw.get("lowDRsize", 23)
    rng = random.Random(L * 131 + low)
    synth_kw = synth_kw or dict(dr_len_min=23, dr_len_max=27)
    base = synth_reads(ca, n_base, read_len=L, crispr_per_million=150000, **synth_kw)
    p = ca.default_params(**kw)
    op = to_orc_params(p)
    ref0 = orc.pipeline(base, params=op, do_pass2=False)
    pats = [bytes(x) for x in ref0.patterns]
    toks = sorted({bytes(t) for t in ref0.tokens if bytes(t) in pats}, key=lambda t: (len(t), t))
    assert toks and len(toks[0]) <= low + 1, "the set must hold short repeats: only they can sit in the last window"
    picked = toks[:6] + toks[-2:]
    seqs, want, cut = list(base), [], []
    for t in picked:
        for o in offsets(L, len(t)):
            assert 0 <= o and o + len(t) <= L
            s = _filler(rng, o) + t + _filler(rng, L - o - len(t))
            want.append(len(seqs)); seqs.append(s)
        s = _filler(rng, L - len(t) + 1) + t[:-1]
        if not any(q in s for q in pats):
            cut.append(len(seqs)); seqs.append(s)
    assert want and cut
    ref = orc.pipeline(seqs, params=op)
    recruited = set(int(r) for r in ref.rec_read[ref.n_pass1:ref.n_pass1 + ref.n_pass2])
    assert all(i in recruited for i in want) and not any(i in recruited for i in cut)
    gpu = ca.search_pipeline(seqs, params=p)
    assert_same_pipeline(gpu, ref)
    got = set(int(r) for r in gpu.rec_read[gpu.n_pass1:gpu.n_pass1 + gpu.n_pass2])
    assert all(i in got for i in want) and not any(i in got for i in cut)
    assert gpu.counters["used_device_merge"] == 1
    return gpu


def _ends(L, n):
    return [L - n - back for back in range(0, 9)]      # the copy ends 0 .. 8 bases before the read's end


@pytest.mark.parametrize("L", [64, 256, 257])
def test_device_built_table_first_and_last_register_forms(ca, L):
    """Rows of 4 and 16 words (the register form's first and last instantiations) and of 17 (the lane-per-read body, W = 0),
    the table built on the device.  Copies at offsets 0 .. 8 and at the read's end.  Two repeats of 23 bases and a spacer of
    26 do not fit into 64 bases, so pass 1 can find nothing in such reads under the default options: that case runs with
    lowSpacerSize = 10 and spacers of 10 .. 14 bases."""
    kw, skw = {}, None
    if L == 64:
        kw, skw = dict(lowSpacerSize=10), dict(dr_len_min=23, dr_len_max=25, spacer_len_min=10, spacer_len_max=14)
    designed_copies(ca, L, 3000, lambda L, n: list(range(0, 9)) + _ends(L, n), kw, skw)


def _round_edge(L, n, first, step):
    """copies whose window is the last of the wave walk's first round and the first of its second, where they fit, and copies at
    the read's end (windows h_max and h_max - 1)"""
    return [o for o in range(first, first + 2 * step) if o + n <= L] + _ends(L, n)


@pytest.mark.parametrize("L", [2056, 2063, 2064])
def test_device_built_table_wave_walk(ca, L):
    """Reads over 800 bases: a wave walks a read, 256 windows a round.  h_max = (L - 16) >> 3 is 255, 255, 256: the read's
    last window is the first round's last, or a second round's only one.  Copies at 2 033 .. 2 048 (windows 255 and 256)
    and at the read's end."""
    designed_copies(ca, L, 1500, lambda L, n: _round_edge(L, n, 2033, 8))


@pytest.mark.parametrize("kw,skw", [(dict(lowDRsize=20, highDRsize=40), dict(dr_len_min=20, dr_len_max=26)),
                                    (dict(lowDRsize=15, searchWindowLength=8), dict(dr_len_min=15, dr_len_max=21))],
                         ids=["ASH=2", "KL=12"])
def test_device_built_table_wave_walk_windows_every_four_bases(ca, kw, skw):
    """Windows every 4 bases: a round is 512 windows = 2 048 bases.  L = 2 080: h_max = (L - KL) >> 2 is 516 (keys of 16 bases)
    and 517 (keys of 12: one more window at the read's end).  Copies at 2 041 .. 2 048 (windows 511 and 512, either side of
    the round's end) and ending 0 .. 8 bases before the read's end (windows h_max - 3 .. h_max)."""
    L = 2080
    KL = 12 if kw["lowDRsize"] < 19 else 16
    assert (L - KL) >> 2 == (517 if KL == 12 else 516)
    skw = dict(skw, n_dr=40, spacer_len_min=26, spacer_len_max=34)
    gpu = designed_copies(ca, L, 1500, lambda L, n: _round_edge(L, n, 2041, 4), kw, skw)
    assert gpu.n_pass2 > 0


def test_per_read_lengths_exception_reads_and_duplicate_headers(ca):
    """The construction of test_gpu_parity's ragged test at 3 000 reads, padded to one stride: per-read lengths (requested a tile
    ahead), header ids (two tiles ahead) whose found flag belongs to a read of another tile, exception reads."""
    rng = random.Random(7)
    base = synth_reads(ca, 3000, read_len=150, crispr_per_million=150000)
    seqs, hdrs = [], []
    for i, s in enumerate(base):
        s = bytearray(s[:rng.randint(40, 150)]) if rng.random() < 0.5 else bytearray(s)
        r = rng.random()
        if r < 0.03:
            s[rng.randrange(len(s))] = ord("N")
        elif r < 0.04:
            for _ in range(5):
                s[rng.randrange(len(s))] = ord("N")
        elif r < 0.045:
            s[rng.randrange(len(s))] = ord("a")
        seqs.append(bytes(s))
        hdrs.append(b"r%d" % (i if rng.random() > 0.05 else rng.randrange(0, i + 1)))
    ref = orc.pipeline(seqs, hdrs)
    gpu = run_one_block(ca, seqs, hdrs, pad_uniform=2)
    assert_same_pipeline(gpu, ref)
    assert gpu.counters["used_fast_filter"] == 1 and gpu.counters["n_exceptions"] > 50
    assert gpu.n_pass2 > 0
    # ... and the same reads through the host-built table, which takes the exception words from the prefetch
    gpu = run_one_block(ca, seqs, hdrs, env={"CRASS_HOST_MERGE": "1"}, pad_uniform=2)
    assert_same_pipeline(gpu, ref)


@pytest.mark.parametrize("kw,env", [(dict(lowDRsize=20, highDRsize=40), {}), (dict(lowDRsize=15, searchWindowLength=8), {}),
                                    ({}, {"CRASS_HOST_MERGE": "1"})],
                         ids=["ASH=2", "KL=12", "host-built table"])
def test_other_instantiations(ca, kw, env):
    """Windows every 4 bases, keys of 12 bases, and k_anchor_filter (host-built table, with_exc = 0), 3 073 reads each."""
    if kw.get("lowDRsize", 23) < 23:
        seqs = synth_reads(ca, 3073, read_len=150, n_dr=40, dr_len_min=kw["lowDRsize"], dr_len_max=kw["lowDRsize"] + 6,
                           spacer_len_min=26, spacer_len_max=34, crispr_per_million=150000)
    else:
        seqs = base_set(ca)[0]
    p = ca.default_params(**kw)
    ref = orc.pipeline(seqs, params=to_orc_params(p))
    gpu = run_one_block(ca, seqs, env=env, params=p)
    assert_same_pipeline(gpu, ref)
    assert gpu.n_pass2 > 0
    assert gpu.counters["used_device_merge"] == (0 if env else 1)


def test_the_switch_is_inert(ca):
    """The same 20 000 reads with the probe's own grid and with one block: identical results."""
    seqs = synth_reads(ca, 20000, read_len=150, crispr_per_million=50000)
    ref = orc.pipeline(seqs)
    plain = ca.search_pipeline(seqs)
    capped = run_one_block(ca, seqs)
    assert_same_pipeline(plain, ref)
    assert_same_pipeline(capped, ref)
    assert_same_pipeline(capped, plain)
    assert plain.n_pass2 > 0
