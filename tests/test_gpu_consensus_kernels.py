"""The consensus stage's two alignment kernels on their own, against the compiled reference's recorded answers
(tests/golden/ref_vectors.json.gz, tests/refvec.py):
* k_cons_ksw (ksw_align with the Aligner's scoring, both orientations of every query) through crass_hip_ksw_batch, on
  the 6 000 short cases of the oracle's pin and on 2 000 queries of 61..320 codes (the striped layout past 64 / 128
  query positions, the kernel's whole LDS range);
* k_cons_sw (smithWaterman) through crass_hip_smith_waterman_batch, which runs the stage's own updateStartStops code
  (scratch layout, chunked launches, Levenshtein batch, similarity decision): every case once, again with a scratch
  budget that forces many chunks, and as one batch of more than 65 536 tasks.
The GPU side reads only the recorded answers, never the reference."""
import pytest

from tests import refvec
from tests.test_oracle_consensus import (KSW_MAX_QLEN, ksw_cases, ksw_live, ksw_long_cases, ksw_long_rc_cases, ksw_rc_cases, sw_cases,
                                         sw_form, sw_live)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


def want_ksw(name, cases):
    """(score, tb, qb) of the recorded (score, te, qe, tb, qb)"""
    return [(w[0], w[3], w[4]) for w in refvec.answers(name, cases, ksw_live)]


def assert_ksw(got, cases, fwd, rev):
    assert got.shape == (len(cases), 2, 3)
    for v, (q, t) in enumerate(cases):
        assert tuple(got[v, 0].tolist()) == fwd[v], ("forward", v, q, t, got[v, 0].tolist(), fwd[v])
        assert tuple(got[v, 1].tolist()) == rev[v], ("reverse complement", v, q, t, got[v, 1].tolist(), rev[v])


def test_ksw_short_queries_both_orientations(ca):
    cases = ksw_cases()
    fwd, rev = want_ksw("ksw_align", cases), want_ksw("ksw_align_rc", ksw_rc_cases())
    got = ca.ksw_batch(cases)                                    # 12 000 alignments: 187.5 blocks of 64 threads
    assert_ksw(got, cases, fwd, rev)
    assert sum(f[0] >= 5 for f in fwd) > 2000 and sum(r[1] >= 0 for r in rev) > 1000
    part = slice(100, 161)                                       # 122 alignments: a partial second block
    assert_ksw(ca.ksw_batch(cases[part]), cases[part], fwd[part], rev[part])


def test_ksw_long_queries_both_orientations(ca):
    cases = ksw_long_cases()
    fwd, rev = want_ksw("ksw_align_long", cases), want_ksw("ksw_align_long_rc", ksw_long_rc_cases())
    assert max(len(q) for q, _ in cases) == KSW_MAX_QLEN
    got = ca.ksw_batch(cases)                                    # 4 000 alignments, 160 KB of LDS per block of 64
    assert_ksw(got, cases, fwd, rev)
    short = [v for v, (q, _) in enumerate(cases) if len(q) <= 128][:37]     # a batch whose LDS stays at 64 KB
    assert len(short) == 37
    assert_ksw(ca.ksw_batch([cases[v] for v in short]), [cases[v] for v in short], [fwd[v] for v in short], [rev[v] for v in short])


def test_ksw_query_over_the_lds_cap_is_refused(ca):
    q = [0, 1, 2, 3] * 80 + [1]                                  # 321 codes
    with pytest.raises(ca.CrassError) as e:
        ca.ksw_batch([([0, 1, 2], [0, 1, 2]), (q, [0, 1, 2, 3] * 10)])
    assert e.value.status == 2                                   # CRASS_ERR_UNSUPPORTED, nothing launched
    with pytest.raises(ca.CrassError) as e:
        ca.ksw_batch([([0, 5], [0, 1])])
    assert e.value.status == 1


def sw_expected(cases):
    return refvec.answers("smith_waterman", cases, sw_live)


def sw_got(cases, out):
    """the batch's (aStart, aEnd, a_off, a_len, b_off, b_len) in the record's form (ret, aStart, aEnd, a_ret, b_ret)"""
    res = []
    for (a, b, s, n, sim), o in zip(cases, out.tolist()):
        a_ret, b_ret = a[o[2]:o[2] + o[3]], b[o[4]:o[4] + o[5]]
        res.append([1 if (sim == 0 or o[3] > 0) else 0, o[0], o[1], a_ret.decode("latin-1"), b_ret.decode("latin-1")])
    return res


def run_sw(ca, cases, idx):
    """cases idx (one similarity) through the batch -> ({case index: record-form answer}, launches)"""
    sims = {cases[k][4] for k in idx}
    assert len(sims) == 1
    out, launches = ca.smith_waterman_batch([cases[k][:4] for k in idx], similarity=sims.pop())
    return dict(zip(idx, sw_got([cases[k] for k in idx], out))), launches


def by_similarity(cases):
    return {sim: [k for k, c in enumerate(cases) if c[4] == sim] for sim in sorted({c[4] for c in cases})}


def assert_sw(cases, want, got):
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, [(k, cases[k][1:], sw_form(cases[k][3], len(cases[k][1])), got[k], want[k]) for k in bad[:5]]


def test_sw_matches_the_reference(ca):
    cases = sw_cases()
    want = sw_expected(cases)
    forms = [0, 0, 0]
    for c in cases:
        forms[sw_form(c[3], len(c[1]))] += 1
    assert min(forms) >= 100, forms                               # LDS wavefront, scratch wavefront, serial
    for sim, idx in by_similarity(cases).items():
        got, launches = run_sw(ca, cases, idx)
        assert launches == 1
        assert_sw(cases, want, got)


def test_sw_in_many_chunks(ca, monkeypatch):
    """the traceback scratch budget (read per call) cut down so that each batch runs in more than 10 launches"""
    cases = sw_cases()
    want = sw_expected(cases)
    monkeypatch.setenv("CRASS_CONS_SW_BUDGET", str(256 * 1024))
    for sim, idx in by_similarity(cases).items():
        got, launches = run_sw(ca, cases, idx)
        assert launches > 10, launches
        assert_sw(cases, want, got)


def test_sw_one_batch_over_65536_tasks(ca):
    """the grid is capped at 16 384 blocks of 4 waves: past 65 536 tasks every wave takes several"""
    cases = sw_cases()
    want = sw_expected(cases)
    idx = by_similarity(cases)[0.85]
    reps = 65536 // len(idx) + 1
    big = idx * reps
    assert len(big) > 65536
    out, launches = ca.smith_waterman_batch([cases[k][:4] for k in big], similarity=0.85)
    assert launches == 1
    got = sw_got([cases[k] for k in big], out)
    bad = [j for j, k in enumerate(big) if got[j] != want[k]]
    assert not bad, [(j, big[j], got[j], want[big[j]]) for j in bad[:5]]


def test_sw_outside_the_reference_domain_is_refused(ca):
    read, dr = b"ACGTACGTAC", b"ACGT"
    for task in [(read, dr, 0, 0), (read, dr, 5, 6), (read, dr, -1, 3), (read, b"", 0, 4)]:
        with pytest.raises(ca.CrassError) as e:
            ca.smith_waterman_batch([(read, dr, 0, 4), task])
        assert e.value.status == 1, task
