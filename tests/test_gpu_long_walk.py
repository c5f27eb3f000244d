"""Pass 1's long-read kernels on the designed reads of tests/walk_sets.py: the light walk (k_long_light, k_long_light_any: hint
words in batches of 64 behind a class switch, the +-24 window of scanRight's first link, the closed-form extension in 64-base
chunks, the lattice test of the every-position form, the survivor-list form of 513 .. 2 048 base sets, a block's second read)
and the wave kernel's own forms (k_survivor: the votes of 2 .. 66 repeats, the match-mask chain over 4 096-base blocks).
Every set goes through search_pipeline and is compared with the oracle field by field; every designed read's record is
compared with the answer written down from its design (test_walk_sets_host.py pins those on the CPU), so no test passes on an
empty answer.  The route switches must not change a record.

What these tests do NOT see: which kernel answered.  The library reports no counter for the route, and a set that fell through
from the light walk to the full wave kernel gives the same records (that is CRASS_NO_LIGHT=1, run here on purpose).  That the
default route of these sets is the light walk rests on engine_pass1.cpp's rule (packed ACGT reads, position hints, no switch
set), not on an assertion here."""
import json
import os
import subprocess
import sys

import pytest

from tests import orc
from tests import walk_sets as W
from tests.parity import assert_same_pipeline
from tests.test_gpu_lane_find import digest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = sorted(W.LIGHT_SETS) + sorted(W.WAVE_SETS)
SWITCHES = {"CRASS_NO_LIGHT": "1", "CRASS_LONG_FULL_LAYOUT": "1", "CRASS_SEQ_WINDOW": "1024", "CRASS_HINT_PARTS": "3"}
SWITCHED = [("batch", "defaults"), ("extend", "defaults"), ("votes", "defaults"), ("masks", "defaults")]

_refs = {}


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


def the_set(kind, draw):
    return W.turns_set(draw) if kind == "turns" else W.gpu_set(kind, draw)


def reference(kind, draw):
    """the oracle's answer, once per set"""
    if (kind, draw) not in _refs:
        _refs[(kind, draw)] = orc.pipeline([r.seq for r in the_set(kind, draw)], params=W.params(draw))
    return _refs[(kind, draw)]


def check(gpu, kind, draw):
    """the oracle's answer, and the designed one read by read"""
    reads = the_set(kind, draw)
    assert_same_pipeline(gpu, reference(kind, draw))
    positives = [i for i, r in enumerate(reads) if r.found]
    assert gpu.n_pass1 == len(positives) > 0 and gpu.rec_read[:gpu.n_pass1].tolist() == positives
    for k, i in enumerate(positives):
        r = reads[i]
        assert (int(gpu.rec_lowlexi[k]), int(gpu.rec_replen[k]), gpu.ss(k)) == (r.low, r.replen, r.ss), r.name


def run(ca, kind, draw):
    gpu = ca.search_pipeline([r.seq for r in the_set(kind, draw)], params=ca.default_params(**W.DRAWS[draw]))
    check(gpu, kind, draw)
    return gpu


@pytest.mark.parametrize("kind,draw", SETS)
def test_a_designed_set(ca, kind, draw):
    gpu = run(ca, kind, draw)
    if kind == "lengths":
        assert gpu.max_read_len == 12289
    if kind == "dense":
        assert 512 < gpu.max_read_len <= 2048


@pytest.mark.parametrize("switch", sorted(SWITCHES))
@pytest.mark.parametrize("kind,draw", SWITCHED)
def test_the_route_switches_keep_the_records(ca, monkeypatch, kind, draw, switch):
    """read per call: the full wave kernel instead of the light walk; every read in the full layout from the start; an ASCII
    window of 1 024 bytes; the hint words computed in three slices"""
    monkeypatch.setenv(switch, SWITCHES[switch])
    run(ca, kind, draw)


def test_a_group_of_two_contexts(ca):
    reads = the_set("batch", "defaults")
    gpu = ca.search_pipeline_group([r.seq for r in reads], [0, 0], local_copies=True)
    gpu.counters = gpu.counters[0]
    check(gpu, "batch", "defaults")


def test_a_blocks_second_read(ca):
    """8 192 + 64 reads: the blocks 0 .. 63 of the light walk take a second read, designed pairs in slots s and s + 8 192"""
    reads = W.turns_set()
    assert len(reads) == W.TURN_SLOTS + 64
    run(ca, "turns", "defaults")


def run_case(kind, draw):
    """one set in this process, against the oracle and the design; prints one JSON line with the result's digest"""
    import crass_amd
    crass_amd.load()
    gpu = run(crass_amd, kind, draw)
    line = dict(kind=kind, draw=draw, n_pass1=int(gpu.n_pass1), n_pass2=int(gpu.n_pass2), digest=digest(gpu))
    print(json.dumps(line), flush=True)
    return line


def in_a_child(cases, env):
    code = "from tests.test_gpu_long_walk import run_case\n" + "".join("run_case(%r, %r)\n" % c for c in cases)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_the_range_form_of_the_light_walk_under_the_defaults():
    """CRASS_HINT_RANGE=2 (read once per process): k_long_light<true> on the default distances"""
    assert "CRASS_HINT_RANGE" not in os.environ
    cases = [("batch", "defaults"), ("extend", "defaults")]
    here = [run_case(*c) for c in cases]
    there = in_a_child(cases, {"CRASS_HINT_RANGE": "2"})
    assert there == here


def test_the_dense_set_without_the_light_walk_over_its_survivors():
    """CRASS_NO_DENSE_LIGHT=1 (read when the context is made): the full wave kernel on the survivor list"""
    assert "CRASS_NO_DENSE_LIGHT" not in os.environ
    cases = [("dense", "defaults"), ("dense", "w7")]
    here = [run_case(*c) for c in cases]
    there = in_a_child(cases, {"CRASS_NO_DENSE_LIGHT": "1"})
    assert there == here
