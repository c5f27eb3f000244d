"""The found-name exchange of a group on the device route (crass_hip_group_set_name_exchange): names written, copied between the
ranks, looked up and marked without crossing to the host, against the reference pipeline and against the host route of the same
group, record for record.  Groups of 2 and 3 contexts share device 0 (local copies); the counters' route word is what keeps a
test from passing through the host route."""
import numpy as np
import pytest

from tests import bgzf_sets, fastx_sets, orc
from tests.parity import assert_same_pipeline

pytestmark = pytest.mark.gpu

N_READS, L = 6000, 150
LONG = b"_" + b"L" * 299                                  # with the number in front of it: a name of more than 300 bytes, the wave kernels'


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def groups(ca):
    made = {}

    def get(n):
        if n not in made:
            made[n] = ca.SearchGroup([0] * n, local_copies=True)
        return made[n]
    yield get
    for g in made.values():
        g.close()


def name_of(j):
    return b"r%d" % j + (LONG if j % 5 == 0 else b"")


@pytest.fixture(scope="module")
def records(ca):
    """the recipe of test_gpu_group_fastx_files.py, cut to 6 000 reads: ragged lengths, N reads, names that repeat inside a file
    and across the two — every fifth of them more than 300 bytes long, so that such names are shared by reads on two ranks"""
    n = N_READS
    spec = ca.synth_spec(read_len=L, crispr_per_million=60000, n_dr=8)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    rng = np.random.default_rng(15)
    out = []
    for i in range(n):
        s = asc[i * L:(i + 1) * L].tobytes()
        if i % 11 == 0:
            s = s[:int(rng.integers(70, L))]
        if i % 501 == 0:
            s = s[:40] + b"N" + s[41:]
        # every 3rd read: the name of a read anywhere in the job, in either file (that read, 1 modulo 3, keeps its own name)
        out.append((name_of(i if i % 3 else (7 * i + 1) % n), s))
    return out


def fq_of(recs):
    return b"".join(b"@" + nm + b" c" + nm[:20] + b"\n" + s + b"\n+\n" + bytes(70 + (k + i) % 40 for i in range(len(s))) + b"\n" for k, (nm, s) in enumerate(recs))


@pytest.fixture(scope="module")
def reference(records):
    seqs, hdrs = [s for _, s in records], [nm for nm, _ in records]
    ref = orc.pipeline(seqs, hdrs)
    assert orc.pipeline(seqs).n_pass2 > ref.n_pass2      # the suppression across names acts on this set
    return ref


def same_results(a, b):
    np.testing.assert_array_equal(a.rec_read, b.rec_read)
    np.testing.assert_array_equal(a.rec_token, b.rec_token)
    assert a.tokens == b.tokens and a.groups == b.groups and a.patterns == b.patterns


def both_routes(g, files, ref, nominal=None, steps=2):
    """the host route's result and counters, then the device route's: the same pipeline, the same three counts, route 1"""
    n = g.n
    g.set_name_exchange(False)
    g.load_fastx_files(files, nominal=nominal)
    g.step()
    host = g.result()
    if ref is not None:
        assert_same_pipeline(host, ref)
    host_cnt = [g.name_exchange_counters(r) for r in range(n)]
    assert all(c[0] == 0 for c in host_cnt)
    g.set_name_exchange(True)
    try:
        g.load_fastx_files(files, nominal=nominal)
        for step in range(steps):                        # (a second step on the same load: buffers sized from the first)
            g.step()
            dev = g.result()
            if ref is not None:
                assert_same_pipeline(dev, ref)
            same_results(dev, host)
            cnt = [g.name_exchange_counters(r) for r in range(n)]
            assert all(c[0] == 1 for c in cnt), cnt
            assert [c[1:] for c in cnt] == [c[1:] for c in host_cnt], (step, cnt, host_cnt)
    finally:
        g.set_name_exchange(False)
    return host_cnt


@pytest.mark.parametrize("n", [2, 3])
def test_the_device_route_equals_the_host_route_and_the_reference(ca, groups, records, reference, n):
    h = len(records) // 2
    files = [fq_of(records[:h]), fq_of(records[h:])]
    cnt = both_routes(groups(n), files, reference)
    assert sum(c[1] for c in cnt) > 100 and sum(c[3] for c in cnt) > 10      # names were published, namesakes found
    for r in range(n):                                   # a rank looks up what the others published
        assert cnt[r][2] == sum(c[1] for q, c in enumerate(cnt) if q != r)
    # among the published names: one of more than 300 bytes that a read on another rank carries too (the wave kernels' work)
    base = ca.fastx_files_shards_host(files, n).rank_read_base
    rank_of = lambda i: int(np.searchsorted(base, i, side="right")) - 1
    by_name = {}
    for i, (nm, _) in enumerate(records):
        by_name.setdefault(nm, []).append(i)
    found = [int(r) for r in groups(n).candidates().read_idx]
    assert any(len(records[r][0]) > 300 and any(rank_of(j) != rank_of(r) for j in by_name[records[r][0]]) for r in found)


def test_the_steps_one_by_one(ca, groups, records, reference):
    """seed scan, merge and recruit as three calls: the answers of the merge's exchange wait on the device for the recruit"""
    h = len(records) // 2
    files = [fq_of(records[:h]), fq_of(records[h:])]
    g = groups(2)
    g.set_name_exchange(True)
    try:
        g.load_fastx_files(files)
        g.seed_scan()
        g.merge()
        assert [g.name_exchange_counters(r)[0] for r in range(2)] == [1, 1]
        g.recruit()
        assert_same_pipeline(g.result(), reference)
    finally:
        g.set_name_exchange(False)


def test_bgzf_files(ca, groups, records, reference):
    h = len(records) // 2
    files = [bgzf_sets.bgzf(fq_of(records[:h])), bgzf_sets.bgzf(fq_of(records[h:]), block=20000)]
    both_routes(groups(3), files, reference, steps=1)


def test_a_rank_without_a_pass_1_record(ca, groups, records):
    """nominal cuts that give the last rank background reads only: it publishes nothing, looks the others' names up and finds its
    namesakes; the others look up nothing of its"""
    import random
    rng = random.Random(4)
    h = len(records) // 2
    front = records[:h]
    # background: reads without a repeat, some of them namesakes of reads in front
    back = [(front[(13 * i) % h][0] if i % 4 == 0 else b"bg%d" % i, fastx_sets.acgt(rng, L)) for i in range(600)]
    f0, f1 = fq_of(front), fq_of(back)
    g = groups(3)
    cnt = both_routes(g, [f0, f1], None, nominal=[len(f0) // 2, len(f0) + 5], steps=1)
    assert cnt[2][1] == 0 and cnt[0][1] > 0 and cnt[1][1] > 0          # the last rank had no pass-1 record
    assert cnt[2][2] == cnt[0][1] + cnt[1][1] and cnt[2][3] > 0         # ... and namesakes of the others' records
    assert cnt[0][2] == cnt[1][1] and cnt[1][2] == cnt[0][1]
    seqs, hdrs = [s for _, s in front + back], [nm for nm, _ in front + back]
    g.set_name_exchange(True)
    try:
        g.load_fastx_files([f0, f1], nominal=[len(f0) // 2, len(f0) + 5])
        g.step()
        assert_same_pipeline(g.result(), orc.pipeline(seqs, hdrs))
    finally:
        g.set_name_exchange(False)


def test_the_switch_from_the_environment(ca, monkeypatch):
    monkeypatch.setenv("CRASS_GROUP_NAMES", "device")
    with ca.SearchGroup([0, 0], local_copies=True) as g:
        monkeypatch.delenv("CRASS_GROUP_NAMES")
        rng = np.random.default_rng(2)
        recs = [(b"n%d" % (i % 40), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 60))) for i in range(80)]
        g.load_fastx_files([fq_of(recs)])
        g.step()
        assert [g.name_exchange_counters(r)[0] for r in range(2)] == [1, 1]
        with pytest.raises(ca.CrassError) as err:
            g.name_exchange_counters(2)
        assert err.value.status == 1
