"""-d 15 .. 18 on the device path: DR strings of 15 to 18 bases take the device merge (dmerge.hip), pass 2's anchor probe with
12-base keys at windows every 4 bases (12 + 4 - 1 = 15: every pattern of >= 15 bases contains one, engine_internal.h, kDevMinDR)
and the exact verification — bit for bit the oracle's records, tokens, groups and pattern sets.  -d 19 and up, and -d 11 .. 14
(host merge + automaton kernels), are pinned where they were."""
import os
import random

import numpy as np
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


def short_set(ca, low, L, n_short=20000, n_default=6000, n_dr=40):
    """reads whose repeats ARE low .. low + 6 bases long, beside default-length ones"""
    seqs = synth_reads(ca, n_short, read_len=L, n_dr=n_dr, dr_len_min=low, dr_len_max=low + 6, spacer_len_min=26, spacer_len_max=34, crispr_per_million=60000)
    seqs += synth_reads(ca, n_default, read_len=L, n_dr=20, crispr_per_million=40000)
    return seqs


def assert_short_path(gpu, low):
    assert gpu.counters["used_device_merge"] == 1
    assert gpu.counters["used_lds_automaton"] == 2          # (2: anchor probe + exact verification)
    assert min(len(t) for t in gpu.tokens) < 19 and gpu.n_pass2 > 0
    if low == 15:
        assert min(len(t) for t in gpu.tokens) < 16         # a member without a sixteenth base: the needle index's cut key


@pytest.mark.parametrize("low", [15, 16, 17, 18])
@pytest.mark.parametrize("L", [101, 150, 300])
def test_repeats_of_15_to_18_bases_take_the_device_merge_and_the_anchor_probe(ca, low, L):
    seqs = short_set(ca, low, L)
    p = ca.default_params(lowDRsize=low, highDRsize=low + 22)
    gpu = ca.search_pipeline(seqs, params=p)
    ref = orc.pipeline(seqs, params=to_orc_params(p))
    assert_same_pipeline(gpu, ref)
    assert_short_path(gpu, low)


@pytest.mark.parametrize("low,L", [(15, 170), (18, 200), (15, 250), (17, 256)])
def test_uniform_strides_of_11_to_16_words(ca, low, L):
    """reads of 161 .. 256 bases in one stride: the register forms of the probe with the most windows per read (up to 62)"""
    seqs = short_set(ca, low, L, 12000, 3000)
    p = ca.default_params(lowDRsize=low, highDRsize=low + 22)
    gpu = ca.search_pipeline(seqs, params=p)
    assert_same_pipeline(gpu, orc.pipeline(seqs, params=to_orc_params(p)))
    assert_short_path(gpu, low)


def rs(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def array_reads(rng, n, L, drs, share=0.06, n_in_repeat=0.0):
    """`share` of the reads carry an array of one of `drs` (15 % of the copies with one changed base, spacers of 26 .. 34 bases,
    a random offset into the array); n_in_repeat: the share of those whose every copy has an 'N' at one position of the repeat"""
    bg = np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(rng.randrange(1 << 30)).randint(0, 4, size=(n, L))]
    out = []
    for i in range(n):
        if rng.random() >= share:
            out.append(bg[i].tobytes())
            continue
        dr = bytearray(rng.choice(drs))
        if rng.random() < n_in_repeat:
            dr[rng.randrange(len(dr))] = ord("N")
        s = bytearray()
        while len(s) < L + 80:
            c = bytearray(dr)
            if rng.random() < 0.15:
                c[rng.randrange(len(c))] = rng.choice(b"ACGT")
            s += c + rs(rng, rng.randint(26, 34))
        at = rng.randrange(0, 60)
        out.append(bytes(s[at:at + L]))
    return out


@pytest.mark.parametrize("low,L", [(15, 150), (17, 101), (16, 300)])
def test_ragged_reads_and_n_bytes_inside_short_repeats(ca, low, L):
    """the 'N' mask with a short key: ragged reads, stray 'N' bytes, and repeats that carry an 'N' in every copy (their strings
    are tokens and patterns with an 'N': the packed key holds an 'A' there, the verification checks the bytes)"""
    rng = random.Random(low * 1000 + L)
    drs = [rs(rng, rng.randint(low, low + 6)) for _ in range(40)]
    p = ca.default_params(lowDRsize=low, highDRsize=low + 22)
    seqs = []
    for q in array_reads(rng, 20000, L, drs, n_in_repeat=0.2) + short_set(ca, low, L, 8000, 2000):
        q = bytearray(q[:rng.randint(max(60, L - 50), L)]) if rng.random() < 0.5 else bytearray(q)
        if rng.random() < 0.02:
            q[rng.randrange(len(q))] = ord("N")
        seqs.append(bytes(q))
    gpu = ca.search_pipeline(seqs, params=p)
    ref = orc.pipeline(seqs, params=to_orc_params(p))
    assert_same_pipeline(gpu, ref)
    assert_short_path(gpu, low)
    assert any(b"N" in t and len(t) < 19 for t in gpu.tokens)


@pytest.mark.parametrize("low,L", [(15, 150), (18, 101)])
def test_a_group_of_two_contexts_on_one_gpu(ca, low, L):
    seqs = short_set(ca, low, L)
    p = ca.default_params(lowDRsize=low, highDRsize=low + 22)
    grp = ca.search_pipeline_group(seqs, [0, 0], params=p, local_copies=True)
    assert_same_pipeline(grp, orc.pipeline(seqs, params=to_orc_params(p)))
    assert min(len(t) for t in grp.tokens) < 19 and grp.n_pass2 > 0


def test_long_reads_walk_the_probe_wave_per_read(ca):
    """reads of 3 to 10 kbp, -d 15: the wave-per-read walk of the probe (a lane takes eight windows of three words) and the
    general form of the verification with 12-base keys"""
    rng = random.Random(15)
    drs = [rs(rng, n) for n in (15, 15, 16, 17, 19, 21)]
    seqs = []
    for i in range(60):
        L = 10000 if i % 3 == 0 else rng.randint(3000, 10000)
        s = bytearray(rs(rng, L))
        if i % 2 == 0:
            dr = rng.choice(drs)
            arr = b"".join(dr + rs(rng, rng.randint(26, 34)) for _ in range(rng.randint(3, 40)))
            at = rng.randint(0, max(0, L - len(arr) - 1))
            s[at:at + len(arr)] = arr
            s = s[:L]
        else:
            # a lone copy or two, anywhere — including the read's last bases (the last window only holds 12 of them)
            dr = rng.choice(drs)
            for at in (rng.randint(0, L - len(dr)), L - len(dr) - rng.randint(0, 3)):
                s[at:at + len(dr)] = dr
        seqs.append(bytes(s))
    # (pure ACGT: a long-read set with an exception read de-duplicates pass 1's strings on the host and keeps the host merge,
    # whatever the options — 'N' bytes with short keys are the ragged test's business)
    p = ca.default_params(lowDRsize=15, highDRsize=37)
    gpu = ca.search_pipeline(seqs, params=p)
    assert_same_pipeline(gpu, orc.pipeline(seqs, params=to_orc_params(p)))
    assert_short_path(gpu, 15)
    assert gpu.n_pass1 >= 10


def both_paths(ca, seqs, p):
    os.environ.pop("CRASS_HOST_MERGE", None)
    dev = ca.search_pipeline(seqs, params=p)
    os.environ["CRASS_HOST_MERGE"] = "1"
    try:
        host = ca.search_pipeline(seqs, params=p)
    finally:
        os.environ.pop("CRASS_HOST_MERGE", None)
    return dev, host


@pytest.mark.parametrize("low,L,k", [(15, 150, 6), (17, 101, 6), (15, 150, 4), (16, 300, 4)])
def test_device_merge_against_host_merge(ca, low, L, k):
    """tokens, groups and patterns in the same ORDER as the host merge's.  A 15-base token has five 11-mers: under the default
    kmer_clust_size of 6 it never joins a group by its own count (yet seeds k-mers that longer tokens hit); under -k 4 it can."""
    seqs = short_set(ca, low, L)
    p = ca.default_params(lowDRsize=low, highDRsize=low + 22, kmer_clust_size=k)
    dev, host = both_paths(ca, seqs, p)
    assert dev.counters["used_device_merge"] == 1 and host.counters["used_device_merge"] == 0
    assert dev.tokens == host.tokens
    assert dev.groups == host.groups
    assert dev.patterns == host.patterns                    # the same ORDER, not just the same set
    assert list(dev.pat_group) == list(host.pat_group)
    np.testing.assert_array_equal(dev.rec_read, host.rec_read)
    np.testing.assert_array_equal(dev.rec_token, host.rec_token)
    np.testing.assert_array_equal(dev.rec_lowlexi, host.rec_lowlexi)
    assert dev.n_pass2 == host.n_pass2
    assert_same_pipeline(dev, orc.pipeline(seqs, params=to_orc_params(p)))
    assert_short_path(dev, low)


@pytest.mark.parametrize("n_dr,kind", [(40, 0), (1600, 1), (12000, 2)])
def test_table_tiers_with_short_keys(ca, n_dr, kind):
    """four 12-base keys per pattern and orientation: exact keys in LDS (up to 2^14 keys), the 2^16-slot fingerprint table (up to
    2^15), Bloom filter + exact keys in L2 beyond"""
    seqs = synth_reads(ca, 120000, read_len=150, n_dr=n_dr, dr_len_min=15, dr_len_max=21, spacer_len_min=26, spacer_len_max=34, crispr_per_million=150000)
    p = ca.default_params(lowDRsize=15, highDRsize=37)
    gpu = ca.search_pipeline(seqs, params=p)
    print("n_dr %d: %d tokens, %d patterns, %d anchor keys, table kind %d" % (n_dr, len(gpu.tokens), gpu.n_patterns, gpu.counters["anchor_keys"],
                                                                               gpu.counters["anchor_table_kind"]))
    assert_same_pipeline(gpu, orc.pipeline(seqs, params=to_orc_params(p)))
    assert gpu.counters["used_device_merge"] == 1 and gpu.counters["used_lds_automaton"] == 2
    assert gpu.counters["anchor_table_kind"] == kind, gpu.counters
    if kind == 1:
        assert (1 << 14) < gpu.counters["anchor_keys"] <= (1 << 15)
    if kind == 2:
        assert gpu.counters["anchor_keys"] > (1 << 15)


@pytest.mark.parametrize("kw", [dict(lowDRsize=14, highDRsize=36, searchWindowLength=7), dict(lowDRsize=11, highDRsize=33, searchWindowLength=6)],
                         ids=["d14w7", "d11w6"])
def test_repeats_below_15_bases_keep_the_host_merge(ca, kw):
    low = kw["lowDRsize"]
    seqs = short_set(ca, low, 150, 12000, 3000)
    p = ca.default_params(**kw)
    gpu = ca.search_pipeline(seqs, params=p)
    assert_same_pipeline(gpu, orc.pipeline(seqs, params=to_orc_params(p)))
    assert gpu.counters["used_device_merge"] == 0 and gpu.counters["used_lds_automaton"] != 2


def test_19_bases_stay_where_they_were(ca):
    seqs = short_set(ca, 19, 150)
    p = ca.default_params(lowDRsize=19, highDRsize=41)
    gpu = ca.search_pipeline(seqs, params=p)
    assert_same_pipeline(gpu, orc.pipeline(seqs, params=to_orc_params(p)))
    assert gpu.counters["used_device_merge"] == 1 and gpu.counters["used_lds_automaton"] == 2


@pytest.mark.parametrize("which,bounds", [(0, "64,0,0,0"), (1, "0,16,0,0"), (2, "0,0,16,0")])
def test_bound_overflows_repeat_cleanly_with_short_keys(ca, which, bounds):
    """the speculation bounds of a context's first call, each too small in turn (CRASS_TEST_BOUNDS): the stage is repeated with
    the exact count, the short keys' results unchanged — bounds[2] is the one the probe's flagged-read count overflows"""
    seqs = short_set(ca, 15, 150)
    p = ca.default_params(lowDRsize=15, highDRsize=37)
    ref = orc.pipeline(seqs, params=to_orc_params(p))
    os.environ["CRASS_TEST_BOUNDS"] = bounds
    try:
        eng = ca.SearchEngine(p)
        try:
            a = ca.search_pipeline(seqs, params=p, engine=eng)
            b = ca.search_pipeline(seqs, params=p, engine=eng)
        finally:
            eng.close()
    finally:
        os.environ.pop("CRASS_TEST_BOUNDS", None)
    assert_same_pipeline(a, ref)
    assert_same_pipeline(b, ref)
    assert b.counters["n_bound_overflows"][which] >= 1 and b.counters["n_merge_fallbacks"] == 0
    assert_short_path(b, 15)
