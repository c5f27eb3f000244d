"""The comment kseq hands on, across the ranks of a group (crass_hip_group_fetch_comments): a rank's shard may begin in the middle
of a file, and the comment carried into it then lies on an earlier rank.  Groups of 1, 2, 3 and 4 contexts on one device (local
copies), nominal cuts such that a file's only comment lies in rank 0's part and the queries in the last rank's, an empty rank in
between, a cut exactly at a file boundary — everything equal to the host function crass_fastx_comments_of on the whole job."""
import numpy as np
import pytest

from tests import comment_sets as cs

pytestmark = pytest.mark.gpu

JOBS = cs.jobs()


def lone(n, at, tag=b"r"):
    """a FASTA file of n two-line records whose only comment sits on record `at`"""
    h = [tag + b"%d" % r for r in range(n)]
    h[at] += b" the only one"
    return cs.fasta(h)


CASES = {
    # name: (files, {ranks: nominal cuts in the job's text space (None: even)})
    "lone_early": ([lone(400, 3)], {1: None, 2: None, 3: None, 4: None}),
    "every_third": (JOBS["every_third"], {2: None, 3: None, 4: None}),
    "three_files": (JOBS["three_files"], {2: None, 3: None, 4: None}),
    "two_files_even": (JOBS["two_files"], {2: None, 4: None}),
    "none": (JOBS["none"], {3: None}),
    "sparse": (JOBS["sparse"], {4: None}),
}


def with_cuts():
    """cases whose cuts are designed: an empty rank in between (two equal nominal cuts), a cut exactly at a file boundary"""
    f = lone(400, 3)
    T = len(f)
    out = {"empty_rank_between": ([f], {3: [T // 2, T // 2], 4: [T // 3, T // 3, T // 3]})}
    a, b = lone(60, 1, b"a"), cs.fasta([b"b%d" % r for r in range(60)])
    out["cut_at_file_boundary"] = ([a, b], {2: [len(a)], 3: [len(a), len(a) + len(b) // 2], 4: [len(a) // 2, len(a), len(a)]})
    c = lone(60, 30, b"c")
    out["comment_behind_the_cut"] = ([b, c], {3: [len(b) + len(c) // 4, len(b) + len(c) * 3 // 4]})
    return out


CASES.update(with_cuts())
PARAMS = [(name, n) for name in sorted(CASES) for n in sorted(CASES[name][1])]


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def groups(ca):
    """one group per number of ranks, made on first use: creating contexts is the expensive part"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = ca.SearchGroup([0] * n, local_copies=True)
        return made[n]
    yield get
    for g in made.values():
        g.close()


@pytest.fixture(scope="module")
def host(ca):
    out = {}
    for name, (files, _) in CASES.items():
        lay = ca.fastx_files_scan_host(files)
        assert lay.accepted, name
        out[name] = (lay, ca.comments_of(cs.arena(files), lay.rec_pos, np.arange(lay.n_reads, dtype=np.uint64), lay.file_read_base))
    return out


@pytest.mark.parametrize("name,n", PARAMS)
def test_group_fetch_equals_the_host_function_on_the_whole_job(ca, groups, host, name, n):
    files, cuts = CASES[name]
    lay, (chars, off, has) = host[name]
    g = groups(n)
    sh = g.load_fastx_files(files, nominal=cuts[n])
    assert sh.n_reads == lay.n_reads, name
    base = sh.rank_read_base
    if name == "lone_early" and n > 1:                   # the only comment lies in rank 0's part, the last rank holds records
        assert int(base[1]) > 3 and int(base[n]) > int(base[n - 1])
    if name == "empty_rank_between":
        assert any(int(base[r + 1]) == int(base[r]) for r in range(1, n - 1)) and int(base[n]) > int(base[n - 1]) and int(base[1]) > 3
    if name == "cut_at_file_boundary":
        assert int(lay.file_read_base[1]) in [int(x) for x in base[1:n]]
    for idx in (list(range(lay.n_reads)), cs.picks(name, lay.n_reads)[:2000], [lay.n_reads - 1], []):
        c, o, h = g.fetch_comments(idx)
        items = [bytes(chars[int(off[r]):int(off[r + 1])]) for r in idx]
        wc, wo = cs.concat(items)
        assert np.array_equal(o, wo) and np.array_equal(c[:int(wo[-1])], wc), (name, n)
        assert np.array_equal(h, has[np.asarray(idx, np.int64)] if len(idx) else has[:0]), (name, n)


def test_argument_and_state_errors(ca, groups):
    g = groups(2)
    g.load_fastx_files(JOBS["every_third"])
    with pytest.raises(ca.CrassError) as err:
        g.fetch_comments([30])
    assert err.value.status == 1
    assert ca.load().crass_hip_group_fetch_comments(g.h, None, 1, None, None) == 1
