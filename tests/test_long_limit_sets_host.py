"""The designed reads of tests/long_limit_sets.py on the oracle (CPU): it finds exactly the placed arrays, with the placed
start/stops, recruits exactly the placed single copies, and nothing else — so a GPU answer that equals the oracle's on this set
(test_gpu_long_reads_limit.py) is never an empty one.  Every expectation below comes from the design, none from a recorded run."""
import pytest

from tests import orc, long_limit_sets as S

DRAWS = {"defaults": {}, "w7_d20_D40": dict(searchWindowLength=7, lowDRsize=20, highDRsize=40)}


def test_the_lengths_of_the_set():
    reads = S.get()
    lens = [r.L for r in reads]
    # the boundary of rows of the read's own length under the defaults, computed from survivor_lds_layout's formula
    print("last length with rows of the read's length: %d (%d bytes), next: %d bytes; bounded rows at 60 000: %d bytes (defaults), "
          "%d bytes (-w 6 -s 8)" % (S.L_OK, S.full_layout_bytes(S.L_OK), S.full_layout_bytes(S.L_OK + 1),
                                   S.full_layout_bytes(60000, row_len=50), S.full_layout_bytes(60000, window=6, low_sp=8, row_len=50)))
    assert 27000 < S.L_OK < 29000
    assert S.full_layout_bytes(S.L_OK) <= S.LDS_BYTES < S.full_layout_bytes(S.L_OK + 1)
    assert S.full_layout_bytes(60000, row_len=50) <= S.LDS_BYTES and S.full_layout_bytes(60000, window=6, low_sp=8, row_len=50) <= S.LDS_BYTES
    for L in (S.L_OK, S.L_OK + 1, 40952, 40953, 59999, 60000, 150, 3000):
        assert L in lens, L
    assert 12 <= sum(L > 2048 for L in lens) <= 20
    # the shapes the routes of the search differ on
    by = {r.name: r for r in reads}
    assert by["many130"].L == 59999 and len(by["many130"].starts) >= 129
    w = by["wide_beyond41000"]
    assert w.starts[0] > 41000 and w.starts[-1] + 30 - w.starts[0] > 4608
    st = by["straddle32768"].starts
    assert st[0] < 32768 < st[-1]
    t = by["tail_at_L"]
    assert t.starts[-1] + 30 == t.L == 60000 and t.starts[0] >= t.L - 200 and len(t.starts) == 3
    t = by["tail_L_OK+1"]
    assert t.L == S.L_OK + 1 and t.starts[0] >= t.L - 200 and len(t.starts) == 3
    assert b"N" in by["straddle32768_N"].seq and b"g" in by["tail_lowercase"].seq
    assert sum(1 for r in reads if set(r.seq) - set(b"ACGT")) == 2
    singles = {r.name: r for r in reads if r.single}
    assert singles["single_at0"].single[1] == 0 and singles["single_beyond32768"].single[1] > 32768
    assert singles["single_ends_at_L"].single[1] + 30 == singles["single_ends_at_L"].L and singles["single_in_60000"].L == 60000
    # a group of two contexts: long reads in both halves
    h = len(reads) // 2
    assert max(lens[:h]) > S.L_OK and max(lens[h:]) == 60000


@pytest.mark.parametrize("draw", sorted(DRAWS))
@pytest.mark.parametrize("max_len", [S.L_OK, S.L_OK + 1, 40952, 40953, 59999, 60000])
def test_oracle_finds_exactly_the_design(draw, max_len):
    reads = S.subset_up_to(S.get(), max_len)
    assert max(r.L for r in reads) == max_len
    res = orc.pipeline([r.seq for r in reads], params=orc.Params.default(**DRAWS[draw]))
    assert res.error == 0
    arrays = [i for i, r in enumerate(reads) if r.dr]
    singles = [i for i, r in enumerate(reads) if r.single]
    assert res.n_pass1 == len(arrays) > 0 and res.rec_read[:res.n_pass1].tolist() == arrays
    for k, i in enumerate(arrays):
        low, ss = reads[i].want_ss()
        assert (int(res.rec_lowlexi[k]), int(res.rec_replen[k]), res.ss(k)) == (low, 30, ss), reads[i].name
    # tokens in order of first appearance, each DR in its low-lexi form; one group each (no k-mer in common)
    forms = []
    for i in arrays:
        f = min(reads[i].dr, S.revcomp(reads[i].dr))
        if f not in forms:
            forms.append(f)
    assert res.tokens == forms and res.groups == [[2 + t] for t in range(len(forms))]
    assert res.patterns == [p for f in forms for p in (f, S.revcomp(f))]
    for k, i in enumerate(arrays):
        assert res.tokens[int(res.rec_token[k]) - 2] == min(reads[i].dr, S.revcomp(reads[i].dr))
    # pass 2: exactly the single copies of a DR that pass 1 found
    recruited = [i for i in singles if min(reads[i].single[0], S.revcomp(reads[i].single[0])) in forms]
    n1 = res.n_pass1
    assert res.n_pass2 == len(recruited) and res.rec_read[n1:].tolist() == recruited
    for k, i in enumerate(recruited):
        low, ss = reads[i].want_single()
        assert (int(res.rec_lowlexi[n1 + k]), res.ss(n1 + k)) == (low, ss), reads[i].name
        assert res.tokens[int(res.rec_token[n1 + k]) - 2] == min(reads[i].single[0], S.revcomp(reads[i].single[0]))
    if max_len == 60000:
        assert len(recruited) == len(singles) == 4 and len(forms) == 2
    # background reads hold no pattern and are recruited by nothing
    for i, r in enumerate(reads):
        if r.background:
            assert not any(p in r.seq for p in res.patterns) and i not in res.rec_read.tolist()
