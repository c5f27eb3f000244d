"""The designed sets of tests/sink_sets.py do what they claim (CPU only): for every layout the oracle's pass-1 reads ARE the
designed F positions and its pass-2 reads ARE the designed R positions (no exception; for the long-read layouts H the designed
reads are found and a random 2 kbp background may be found too), S reads pass the lattice test, Z, R and V reads fail the padded
model every filter lies inside, and every boundary a layout lists has a record just below it and on it.  That is the argument
that a record dropped, doubled or shifted at one of these boundaries on the GPU shows in the arrays test_gpu_sinks.py compares.
One line per layout: n, survivors (F + S), found, distinct (tokens of pass-1 records), hits (R + V), recruits."""
import numpy as np
import pytest

from tests import edge_reads as E
from tests import sink_sets as S

NAMES = list(S.LAYOUTS)


def _padded_any(lay, idx):
    """does the padded model hold for any of the reads idx (in chunks: a million rows do not fit one table)"""
    rows = lay.rows()
    for lo in range(0, len(idx), 65536):
        if E.padded_model_batch(rows[idx[lo:lo + 65536]], S.P).any():
            return True
    return False


@pytest.mark.parametrize("name", NAMES)
def test_a_layout(name):
    lay, r = S.layout(name), S.reference(name)
    assert r.error == 0
    p1 = np.asarray(r.rec_read[:r.n_pass1], np.int64)
    p2 = np.asarray(r.rec_read[r.n_pass1:r.n_pass1 + r.n_pass2], np.int64)
    assert (np.diff(p1) > 0).all() and (np.diff(p2) > 0).all()
    tok1 = np.asarray(r.rec_token[:r.n_pass1], np.int64)
    print("%-16s n %8d  survivors %7d  found %7d  distinct %5d  hits %7d  recruits %7d" % (
        name, lay.n, len(lay.F) + len(lay.S), r.n_pass1, len(np.unique(tok1)), len(lay.R) + len(lay.V), r.n_pass2))
    assert len(lay.F) + len(lay.S) + len(lay.Z) + len(lay.R) + len(lay.V) == lay.n
    if lay.exact:
        np.testing.assert_array_equal(p1, lay.F)
        np.testing.assert_array_equal(p2, lay.R)
        for i in lay.S:
            assert E.lattice_hit(lay.read(int(i)), S.P), i
        assert not _padded_any(lay, np.concatenate([lay.Z, lay.R, lay.V]))
    else:
        assert np.isin(lay.F, p1).all()
    # a record just below every listed boundary and on it
    surv = np.sort(np.concatenate([lay.F, lay.S]))
    hits = np.sort(np.concatenate([lay.R, lay.V]))
    _, first = np.unique(tok1, return_index=True)
    for space, lo, hi in lay.bounds:
        assert hi == lo + 1
        for k in (lo, hi):
            if space == "read":
                assert k in p1, (space, k)
            elif space == "surv":
                assert surv[k] in p1, (space, k)
            elif space == "cand":
                assert k in first, (space, k)
            else:
                assert space == "hit" and hits[k] in p2, (space, k)


def test_layout_sizes_rest_on_the_stated_constants():
    n = S.first_n_with_look()
    assert n == 699052 and S.survivor_bound(n) > (1 << 20) >= S.survivor_bound(n - 1)
    assert S.layout("D1").n == 65 * 1024 + 1 and S.layout("D2").n == 2049 and S.layout("P2").n == S.N_P_FRONT + 65 * 4096 + 1
    assert [S.lookback_tile_words((m + 63) // 64) for m in S.M2_N] == [256, 4096, 4096]
    assert [-(-((m + 63) // 64) // S.lookback_tile_words((m + 63) // 64)) for m in S.M2_N] == [64, 4, 5]
    assert [-(-((m + 63) // 64) // 256) for m in S.M1_N] == [1, 1, 2, 3] and [m % 64 for m in S.M1_N] == [63, 0, 1, 1]
    assert S.edges(16384, 49152) == [0, 1, 63, 64, 1023, 1024, 16383, 16384, 16385, 49152]


@pytest.mark.parametrize("name", ["D1", "D2"])
def test_tokens_in_the_designed_first_occurrence_order(name):
    lay, r = S.layout(name), S.reference(name)
    assert [bytes(t) for t in r.tokens] == lay.tokens and len(set(lay.tokens)) == len(lay.tokens)
    tok = np.asarray(r.rec_token[:r.n_pass1], np.int64)
    _, first = np.unique(tok, return_index=True)
    if name == "D1":
        a, b = lay.ab
        assert sorted(first.tolist()) == [0] + [x for x in S.D1_RANKS if x != b]
        assert tok[a] == tok[b] and r.rec_lowlexi[a] != r.rec_lowlexi[b]
        assert S.revcomp(lay.read(a)) == lay.read(b)
    else:
        assert sorted(first.tolist()) == list(range(1024)) + [2048]
        np.testing.assert_array_equal(tok[1024:2048], tok[:1024][::-1])


def test_the_vectorised_comparison_sees_what_the_loop_sees():
    """assert_same_arrays against parity.assert_same_pipeline on one small set: both accept the answer itself, and both refuse a
    dropped record, a doubled one, a changed start/stop and a swapped pair of tokens"""
    import copy
    from tests.parity import assert_same_pipeline
    r = S.reference("P1-4095-alt")
    assert r.n_pass1 and r.n_pass2
    S.assert_same_arrays(r, r)
    assert_same_pipeline(r, r)

    def drop(x):
        k = x.n_pass1 + 5
        for f in ("rec_read", "rec_lowlexi", "rec_token", "rec_replen", "rec_nss", "rec_ss_off"):
            setattr(x, f, np.delete(getattr(x, f), k))
        x.n_pass2 -= 1

    def double(x):
        k = x.n_pass1 + 5
        for f in ("rec_read", "rec_lowlexi", "rec_token", "rec_replen", "rec_nss", "rec_ss_off"):
            setattr(x, f, np.insert(getattr(x, f), k, getattr(x, f)[k]))
        x.n_pass2 += 1

    def stop(x):
        x.ss_pool = x.ss_pool.copy()
        x.ss_pool[int(x.rec_ss_off[x.n_pass1 - 1]) + 1] += 1

    def swap(x):
        x.tokens = [x.tokens[1], x.tokens[0]] + list(x.tokens[2:])

    for slip in (drop, double, stop, swap):
        bad = copy.deepcopy(r)
        slip(bad)
        for check in (S.assert_same_arrays, assert_same_pipeline):
            with pytest.raises(AssertionError):
                check(bad, r)
