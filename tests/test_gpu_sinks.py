"""The ordered sinks of both passes (sinks.hip: launch_compact / k_mask_compact_lb and the three-kernel form, k_found_compact,
k_gather_found, k_dr_dedupe_*, k_dx_flag_compact / k_dx_assign_gather, k_valid_compact / k_pack_p2_blob, and the long-read host
loop's k_select_found -> compaction -> k_gather_sparse) on the designed dense sets of tests/sink_sets.py.  Every case is the
WHOLE set against orc.pipeline, field by field (sink_sets.assert_same_arrays); test_sink_sets_host.py shows on the CPU that each
set has a record on both sides of every tile, block and word boundary it names, so a record dropped, doubled or shifted there
changes the compared arrays.

A set the engine answers through a fallback (n_merge_fallbacks, a stage repeated after an overflowed bound) is a pass: the
route is printed next to the case, one JSON line per case with the counters and the wall time of each step.

What these tests do NOT see: that pass 2's probe flags a V read (by construction of the read; the library reports no per-read
flag), and which kernel form answered beyond what the counters say."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import sink_sets as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE = ("n_bound_overflows", "used_device_merge", "n_merge_fallbacks", "n_filter_survivors", "n_pass1_found", "n_pass2_found")
IN_TURN = ("M1-16385", "D1", "M1-16383", "F1-16385-allS", "P1-4097-alt", "D2", "M1-32769")
OTHER_FORMS = ("M1-16385", "F1-16385-edges", "F1-49153-mid", "D1", "D2", "P1-4097-edges", "P1-12289-mid", "H-edges", "H-alt")
PER_CONTEXT = ("CRASS_NO_LOOKBACK", "CRASS_DD_FULL_TABLE", "CRASS_NO_SPECULATION")      # read when a context is created
PER_PROCESS = ("CRASS_P2_BLOB12", "CRASS_SINK_EAGER")                                   # read once per process


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


def new_engine(ca, env=None):
    """a context of its own; the switches are set only while it is created (they are read then)"""
    env = dict(env or {})
    os.environ.update(env)
    try:
        return ca.SearchEngine()
    finally:
        for k in env:
            os.environ.pop(k, None)


def one_step(eng):
    """seed scan, merge, recruit on the resident set -> the result in the oracle's field names"""
    from crass_amd.engine import PipelineResult
    cand = eng.seed_scan()
    eng.merge(fetch=False)
    rec = eng.recruit()
    res = PipelineResult(cand, eng.merge_view(), rec, cand.max_read_len)
    res.counters = eng.counters()
    return res


def run_layout(ca, eng, name, steps, label=""):
    """load the layout into the context, run `steps` steps, compare every one with the layout's own oracle answer"""
    lay, ref = S.layout(name), S.reference(name)
    packed = ca.PackedReads(lay.reads, 2)
    times = []
    try:
        t0 = time.perf_counter()
        eng.load_reads(packed)
        times.append(round(time.perf_counter() - t0, 3))
        for _ in range(steps):
            t0 = time.perf_counter()
            gpu = one_step(eng)
            times.append(round(time.perf_counter() - t0, 3))
            t0 = time.perf_counter()
            S.assert_same_arrays(gpu, ref)
            c = gpu.counters
            assert c["n_pass1_found"] == ref.n_pass1 and c["n_pass2_found"] == ref.n_pass2, c
            if name.startswith(("M1", "F1")):
                assert c["n_filter_survivors"] == len(lay.F) + len(lay.S), c
            times.append(round(time.perf_counter() - t0, 3))
    finally:
        packed.close()
    line = dict(case=name, form=label, n=lay.n, load_step_check_s=times, **{k: c[k] for k in ROUTE})
    print(json.dumps(line), flush=True)
    return gpu


@pytest.mark.parametrize("name", list(S.LAYOUTS))
def test_a_layout_on_a_fresh_context(ca, name):
    """three steps: the first on presized bounds (a dense set overflows the survivor bound and the stage is repeated with the
    exact count), the later ones on bounds learnt from the step before"""
    with new_engine(ca) as eng:
        run_layout(ca, eng, name, 3)


def test_one_context_sets_in_turn(ca):
    """The ticket's self-reset and the epoch across launches of different tile counts, a status array that grows and is zeroed
    again between loads, bounds learnt on a dense set and met by a sparse one and the reverse: two steps per set, every result
    against its own oracle"""
    with new_engine(ca) as eng:
        for name in IN_TURN:
            run_layout(ca, eng, name, 2, "in turn")


@pytest.mark.parametrize("switch", PER_CONTEXT)
@pytest.mark.parametrize("name", OTHER_FORMS)
def test_the_other_forms(ca, name, switch):
    """the three-kernel compactions, the de-duplication table sized for the records, every stage sized from exact counts"""
    assert switch not in os.environ
    with new_engine(ca, {switch: "1"}) as eng:
        run_layout(ca, eng, name, 2, switch)


def run_other_forms(label):
    """the subset in this process (a child started with a per-process switch set)"""
    import crass_amd
    crass_amd.load()
    for name in OTHER_FORMS:
        with new_engine(crass_amd) as eng:
            run_layout(crass_amd, eng, name, 2, label)
    print("other forms ok", flush=True)


_child_failed = []


@pytest.mark.parametrize("switch", PER_PROCESS)
def test_the_other_forms_in_a_child(switch):
    """the 12-byte pass-2 record and the eager sink: read once per process, so each runs the subset in one child process"""
    assert switch not in os.environ
    assert not _child_failed, "an earlier child failed (%s): no second one is started" % _child_failed
    code = "from tests.test_gpu_sinks import run_other_forms\nrun_other_forms(%r)\n" % switch
    try:
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **{switch: "1"}), capture_output=True, text=True,
                           timeout=300)
    except subprocess.TimeoutExpired:
        _child_failed.append(switch)
        raise
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            print(ln)
    if r.returncode != 0 or "other forms ok" not in r.stdout:
        _child_failed.append(switch)
    assert r.returncode == 0 and "other forms ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
