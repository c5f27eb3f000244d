"""CPU checks of the edge-read generator (tests/edge_reads.py) and of its padded superset model against the oracle.  The GPU
side, tests/test_gpu_filter_edges.py, runs these sets through every route of the pass-1 seed filter."""
import numpy as np
import pytest

from tests import edge_reads as E
from tests import orc

OPTION_SETS = {
    "defaults": {},
    "s20S60": dict(lowSpacerSize=20, highSpacerSize=60),
    "w6": dict(searchWindowLength=6),
    "w7": dict(searchWindowLength=7),
    "w9": dict(searchWindowLength=9),
    "d20D40": dict(lowDRsize=20, highDRsize=40),
    "d15": dict(lowDRsize=15),
    "d30D60": dict(lowDRsize=30, highDRsize=60),
}
LENGTHS = (64, 101, 150, 256, 300, 1000)
S_LENGTHS = (150, 256, 300, 1000, 3000)
S_OPTION_SETS = ("defaults", "d20D40")


def _key(name):
    return E.key(E.params(**OPTION_SETS[name]))


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_positive_and_negative_sets(name, L):
    """P: every read is oracle-positive (a planted exact copy at an edge pair).  N: every read is false under the padded model
    and oracle-negative.  (params, L) without a seed that fits give empty sets."""
    k = _key(name)
    p = orc.Params(*k)
    P, N = E.positive_set(k, L), E.negative_set(k, L)
    if not E.has_seed(p, L):
        assert P == [] and N == []
        return
    s = E.shape(p, L)
    print(name, L, s, "P", len(P), "N", len(N))
    assert len(P) >= 8 and len(N) >= 8
    assert all(len(r) == L and set(r) <= set(b"ACGT") for r in P + N)
    assert all(E.lattice_hit(r, p) == 1 for r in P)
    assert all(E.padded_model(r, p) for r in P)
    assert not E.padded_model_batch(np.frombuffer(b"".join(N), np.uint8).reshape(len(N), L), p).any()
    assert all(E.lattice_hit(r, p) == 0 for r in N)
    # the edges themselves are planted: the last lattice seed, and dmax for it
    last = s.skips * (s.searchEnd // s.skips)
    assert last in E.edge_seeds(s) and E.dmax(s, last) in E.edge_distances(s, last)


@pytest.mark.parametrize("L", [58, 64, 75, 100, 101, 137, 150, 200, 250, 256, 257, 258, 265, 300])
def test_last_seed_on_search_end_and_dmax_clamp(L):
    """defaults: where searchEnd is a multiple of 8 the last lattice seed IS searchEnd (58, 250, 258, ...); the distances of
    every seed stop at the reference's clamp, a copy ending at base L - 2"""
    s = E.shape(E.params(), L)
    js = E.edge_seeds(s)
    assert js[-1] == 8 * (s.searchEnd // 8) and (js[-1] == s.searchEnd) == (s.searchEnd % 8 == 0)
    for j in js:
        ds = E.edge_distances(s, j)
        assert ds[0] == s.D0 and ds[-1] == E.dmax(s, j) and j + ds[-1] + s.w == min(L - 1, j + s.D1 + s.w)


@pytest.mark.parametrize("L", S_LENGTHS)
@pytest.mark.parametrize("name", S_OPTION_SETS)
def test_class_switch_set(name, L):
    """S: at least 200 reads per length, each (a) found by the oracle after at least one class switch and (b) with a record
    that differs from the one for the same read without the decoy (so a walk that skips the switch cannot pass)"""
    k = _key(name)
    p = orc.Params(*k)
    S, twins, tried = E.class_switch_set(k, L)
    print(name, L, "kept", len(S), "of", tried)
    assert len(S) >= 200 and len(twins) == len(S)
    for r, t in zip(S, twins):
        assert len(r) == len(t) == L and sum(x != y for x, y in zip(r, t)) <= E.shape(p, L).w
        E.class_switches(reset=True)
        rec = orc.search_core(r, p)
        assert rec[0] == 1 and E.class_switches()[1] >= 1
        assert orc.search_core(t, p) != rec


@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_oracle_lattice_hit_implies_padded_model(name):
    """20 000 random reads per option set, lengths 64 .. 300: orc_has_lattice_hit => padded_model (inputs the generator did not
    shape)"""
    k = _key(name)
    p = orc.Params(*k)
    rng = np.random.default_rng(list(k) + [7])
    n_hit = n_model = 0
    for L in (64, 101, 150, 256, 300):
        a = E.LETTERS[rng.integers(0, 4, size=(4000, L))]
        model = E.padded_model_batch(a, p)
        oracle = np.array([E.lattice_hit(a[i].tobytes(), p) for i in range(len(a))])
        assert set(oracle.tolist()) <= {0, 1}
        assert not np.any((oracle == 1) & ~model), (L, np.flatnonzero((oracle == 1) & ~model)[:5])
        n_hit += int(oracle.sum())
        n_model += int(model.sum())
    print(name, "oracle hits", n_hit, "model", n_model)
    assert n_hit > 0


def test_exact_filter_model_implies_padded_model():
    """defaults at 150 bases: the exact predicate of tests/test_gpu_filter_pairs.py lets through no read the padded model
    rejects, on random reads and on its adversarial reads"""
    from tests.test_gpu_filter_pairs import adversarial_reads, exact_filter_model
    p = E.params()
    rng = np.random.default_rng(8)
    rand = [r.tobytes() for r in E.LETTERS[rng.integers(0, 4, size=(20000, 150))]]
    adv, _ = adversarial_reads()
    for seqs in (rand, adv):
        exact = exact_filter_model(seqs)
        model = E.padded_model_batch(np.frombuffer(b"".join(seqs), np.uint8).reshape(len(seqs), 150), p)
        print("exact", int(exact.sum()), "padded", int(model.sum()), "of", len(seqs))
        assert not np.any(exact & ~model)
        assert exact.sum() > 0
