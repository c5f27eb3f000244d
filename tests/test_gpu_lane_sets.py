"""The lane kernel's stages behind its seed find (k_survivor_lanes, crass_amd/csrc/survivor_lanes.hip) on the designed twin pairs
of tests/lane_sets.py: the pooled QC (the threshold tests (double)similarity > 0.82 of two and three repeats as queued tasks, d_no
and the early stop of ln_lev_regs, 32-bit tasks from the queue's front and 64-bit ones from its back, the QcTask bit fields,
the length cut-offs 12 / 30 and the spacer bounds, isRepeatLowComplexity by bit planes), ln_extend2 and ln_extend, and the inline
DRLowLexi.  Every set goes through search_pipeline and is compared with the oracle field by field, and every designed read's
record with the answer written down from its design (tests/test_lane_sets_host.py pins those on the CPU), so nothing passes on
an empty answer.  The sets then run in fresh child processes (the switches are read once per process) with
CRASS_NO_LANE_KERNEL=1 — the wave kernel's packed_similarity, narrow and wide, and its own orientation — and with
CRASS_SURV_NO_REGROUP=1, the lanes in slot order: both must give the parent's records.

What these tests do NOT see: which kernel answered a read.  The library reports no counter for the lane kernel's hand-overs;
that no designed read is handed to the wave kernel rests on the code and on the lengths test_lane_sets_host.py asserts.

DO THE TESTS BITE?  Checked once, not part of the suite: each slip below was applied to a scratch copy of the kernel sources (one
line each; none can fault), the library rebuilt and every set run against it, the records compared with the designed answers
read by read.  The unmodified kernel changes no read.  Slip by slip, the kinds whose designed reads change and the sets:
  `cut_off` compared with >= (isRepeatLowComplexity)   low_complexity: 24 reads of L150 — the found twin of every pair — and 20 of ragged
  `> 12` as `>= 12` in qc_pool_end                     lengths: 6 reads each of L251 and L400 (three_s1_s2_13, three_s2_s1_13)
  qc_pool_end ignoring slot_b                          sim3 (rs and both_b twins): 4 .. 20 reads of every set that holds the kind
  max_right one short at the read's end (ln_extend2)   extend2 second_ends_at_L-1|2 in L150, L251, D75, ragged; field_edges ends_at_L-1
                                                       (10 reads of L512); the orientation twins whose array ends with the read
  `drop < 64` as `drop <= 64` in the orientation       every found read with a repeat of 32 bases, in all eleven sets (orientation
                                                       n32_*, sim2 / words / sim3 / low_complexity / second_round / field_edges n32, pool)
  the transposition term in cell (2, 2) too            transposition: the found twin of all six pairs, in L150 and in L251; three sim2 reads
      (`j < 1` AND the mask ~1: what `j < 2` guards)
  the early stop one column EARLY (m - 2 - j)          sim2, words, transposition, sim3, second_round, field_edges: 69 .. 152 reads a set
  d_no one too SMALL in qc_enqueue_above               every found read of two and three repeats of every set
and the slips that change nothing, with the reason no accepted array can depend on them:
  `> 0.82` as `>= 0.82` in qc_run_task                 the left side is a float widened to double, and no float equals the double
                                                       0.82: the two comparisons agree on every value
  d_no one too LARGE in qc_enqueue_above               d_no only tells ln_lev_regs when it may stop; a later stop returns the exact
                                                       distance or a value >= d_no, and the verdict is taken from that value again
                                                       (the other direction, above, fails everything)
  the early stop as dist - (m - j) >= stop_at          one column LATE: the same, it returns what the full loop returns
  `if (j < 2) TR = 0` as `j < 1` alone                 the cell (i, 2) is offered M[i-2][0] + 1 = i - 1, which the plain recurrence
                                                       reaches there already (lane_sets' text); only with the mask opened as
                                                       well, cell (2, 2), does a distance change (above)
  max_left without the spacing - len_r bound           a left run beyond the bound means the copies agree over the whole spacing: a
                                                       spacer of 0 bases, rejected either way, and the next seed is taken from
                                                       the last STOP, which no left run moves
  `pick` always 2                                      with two repeats both copies get the same two runs and neither clamp of the
                                                       start/stops binds: lenA == lenB, and the rule picks the second repeat
"""
import json
import os
import subprocess
import sys

import pytest

from tests import orc
from tests import lane_sets as S
from tests.parity import assert_same_pipeline
from tests.test_gpu_lane_find import digest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = {"CRASS_NO_LANE_KERNEL": "1", "CRASS_SURV_NO_REGROUP": "1"}
FILTER = {150: 1, 400: 2, 512: 2}           # used_fast_filter by read length: lane per read, wave per read

_refs, _lines = {}, {}


def reference(name):
    """the oracle's answer, once per set"""
    if name not in _refs:
        _refs[name] = orc.pipeline([r.seq for r in S.the_set(name)], params=S.params(S.draw_of(name)))
    return _refs[name]


def check(gpu, name):
    """the oracle's answer, and the designed one read by read"""
    reads = S.the_set(name)
    assert_same_pipeline(gpu, reference(name))
    positives = [i for i, r in enumerate(reads) if r.found]
    assert gpu.n_pass1 == len(positives) > 0 and gpu.rec_read[:gpu.n_pass1].tolist() == positives
    wrong = []
    for k, i in enumerate(positives):
        r = reads[i]
        if (int(gpu.rec_lowlexi[k]), int(gpu.rec_replen[k]), gpu.ss(k)) != (r.low, r.replen, r.ss):
            wrong.append(r.name)
    assert not wrong, wrong
    L = S.PLANS[name][1] if name in S.PLANS else None
    if L in FILTER and S.draw_of(name) == "defaults":
        assert gpu.counters["used_fast_filter"] == FILTER[L], gpu.counters
    # every designed read holds a seed with a copy in its window (found, or a rejected candidate): the filter lets it through
    designed = sum(r.kind != "background" for r in reads)
    assert gpu.counters["n_filter_survivors"] >= designed > 0, (gpu.counters["n_filter_survivors"], designed)


def run_case(name, against_the_oracle=True):
    """one set in this process; prints one JSON line with the result's digest"""
    import crass_amd as ca
    ca.load()
    reads = S.the_set(name)
    gpu = ca.search_pipeline([r.seq for r in reads], params=ca.default_params(**S.DRAWS[S.draw_of(name)]))
    if against_the_oracle:
        check(gpu, name)
    line = dict(set=name, n=len(reads), n_pass1=int(gpu.n_pass1), n_pass2=int(gpu.n_pass2), digest=digest(gpu))
    print(json.dumps(line), flush=True)
    return line


def here(name):
    if name not in _lines:
        _lines[name] = run_case(name)
    return _lines[name]


@pytest.mark.parametrize("name", S.SETS)
def test_a_designed_set(name):
    assert not set(SWITCHES) & set(os.environ)
    line = here(name)
    assert line["n_pass1"] > 0


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_a_switch_keeps_the_records(switch):
    """every set again in ONE fresh child process with the switch set; a non-zero exit fails the test"""
    assert not set(SWITCHES) & set(os.environ)
    mine = [here(name) for name in S.SETS]
    code = "from tests.test_gpu_lane_sets import run_case\n" + "".join("run_case(%r, False)\n" % name for name in S.SETS)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **{switch: SWITCHES[switch]}), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    there = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert there == mine, [(a["set"], a["n_pass1"], b["n_pass1"]) for a, b in zip(there, mine) if a != b]
