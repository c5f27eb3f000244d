"""Every route of the pass-1 seed filter, read by read on the edge sets of tests/edge_reads.py.

P (one exact copy of one lattice seed at an edge pair) must survive whole: n_filter_survivors == len(P), and since survivors
are at most the reads, no read of P was dropped.  N (near misses, padded-model-negative) must not: n_filter_survivors == 0,
so a filter that passes everything cannot satisfy the P check.  used_fast_filter names the route's family (1 lane-per-read,
2 hint bits, 0 k_filter_general), so a routing change cannot move the coverage elsewhere quietly.  P and N are ACGT only:
exception reads always count as survivors.  Then the array set A and the class-switch set S run through the whole pipeline
and must equal the oracle field by field.

CRASS_FF_RPL, CRASS_FF_EXACT and CRASS_HINT_RANGE are read once per process: those routes run in a fresh child process."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import edge_reads as E
from tests import orc
from tests.parity import assert_same_pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LCT_LENGTHS = (100, 101, 125, 126, 150, 151, 250, 251)
HINT_LENGTHS = (257, 258, 265, 300, 512, 513, 1000, 2048)
RAGGED_256 = ((100, 150, 200, 256),)                   # strides differ, tight layout: no lane-per-read filter
TRIMMED = ((140, 145, 150, 155, 160),)                 # padded to one stride (pad_uniform=2): per-lane searchEnd

# id: (options, lengths (an int: one uniform set; a tuple: one set of those lengths), pad_uniform, in-process env,
#      child-process env, used_fast_filter)
# (every route has a length whose last lattice seed is searchEnd itself: 250 / 58 / 100 / 106 / 65 / 154 / 152 / 147 / 149 /
#  150 / 155 / 258 / 307)
ROUTES = {
    "fast_impl_lct": ({}, LCT_LENGTHS, 0, {}, None, 1),
    "fast_pairs_rpl4": ({}, LCT_LENGTHS, 0, {}, {"CRASS_FF_RPL": "4"}, 1),
    "fast_impl_lct_rpl4": ({}, LCT_LENGTHS, 0, {}, {"CRASS_FF_RPL": "4", "CRASS_FF_EXACT": "1"}, 1),
    "fast_impl_generic": ({}, (58, 64, 75, 137, 200, 256) + TRIMMED, 2, {}, None, 1),
    "fast_range_s20S60": (dict(lowSpacerSize=20, highSpacerSize=60), (64, 100, 150, 252), 0, {}, None, 1),
    "fast_range_S48": (dict(highSpacerSize=48), (106, 150), 0, {}, None, 1),             # D1 = 95 = 16 * 5 + 15
    "fast_range_D0_32": (dict(lowSpacerSize=9), (65, 150), 0, {}, None, 1),
    "fast_range_S90": (dict(highSpacerSize=90), (150, 154), 0, {}, None, 1),             # D1 = 137 > 127
    "fast_any_w6": (dict(searchWindowLength=6), (150, 152), 0, {}, None, 1),
    "fast_any_w7": (dict(searchWindowLength=7), (147, 150), 0, {}, None, 1),
    "fast_any_w9": (dict(searchWindowLength=9), (149, 150), 0, {}, None, 1),
    "fast_any_d20D40": (dict(lowDRsize=20, highDRsize=40), (150, 256), 0, {}, None, 1),   # skips 5
    "fast_any_d15": (dict(lowDRsize=15), (150, 256), 0, {}, None, 1),                     # skips 1: more than 32 seeds
    "fast_any_d30D60": (dict(lowDRsize=30, highDRsize=60), (150, 155), 0, {}, None, 1),   # skips 15
    "hint_positions": ({}, HINT_LENGTHS + RAGGED_256, 0, {}, None, 2),
    "hint_positions_range": (dict(lowSpacerSize=20, highSpacerSize=60), (300, 1000), 0, {}, None, 2),
    "hint_positions_range_env": ({}, (258, 300, 1000), 0, {}, {"CRASS_HINT_RANGE": "1"}, 2),
    "hint_filter_any_w7": (dict(searchWindowLength=7), (300, 307, 1000), 0, {}, None, 2),
    "hint_filter_any_d20D40": (dict(lowDRsize=20, highDRsize=40), (300, 1000), 0, {}, None, 2),
    "general_no_hint_filter": ({}, HINT_LENGTHS + RAGGED_256, 0, {"CRASS_NO_HINT_FILTER": "1"}, None, 0),
    "general_S90": (dict(highSpacerSize=90), (300,) + RAGGED_256, 0, {}, None, 0),
}


def _sets(fn, key, lengths):
    """[(label, reads)] for one entry of a route's lengths"""
    if isinstance(lengths, int):
        return [(str(lengths), fn(key, lengths))]
    return [("+".join(map(str, lengths)), [r for L in lengths for r in fn(key, L)])]


def _params(ca, kw):
    p = ca.default_params(**kw)
    op = orc.Params(p.lowDRsize, p.highDRsize, p.lowSpacerSize, p.highSpacerSize, p.searchWindowLength, p.minNumRepeats,
                    p.kmer_clust_size)
    return p, op


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_route(rid):
    """P, N and A of one route; prints one JSON line per set"""
    import crass_amd as ca
    ca.load()
    kw, lengths, pad, env, _child_env, want_route = ROUTES[rid]
    p, op = _params(ca, kw)
    key = E.key(op)
    n_sets = 0
    for entry in lengths:
        for label, P in _sets(E.positive_set, key, entry):
            _, N = _sets(E.negative_set, key, entry)[0]
            _, A = _sets(E.array_set, key, entry)[0]
            if not P:
                continue
            n_sets += 1
            for name, seqs, want in (("P", P, len(P)), ("N", N, 0)):
                t = time.time()
                g = _with_env(env, lambda: ca.search_pipeline(seqs, params=p, do_pass2=False, pad_uniform=pad))
                c = g.counters
                print(json.dumps({"route": rid, "L": label, "set": name, "n": len(seqs), "survivors": int(c["n_filter_survivors"]),
                                  "used_fast_filter": int(c["used_fast_filter"]), "s": round(time.time() - t, 3)}), flush=True)
                assert c["n_exceptions"] == 0
                assert c["used_fast_filter"] == want_route, (rid, label, name, c["used_fast_filter"])
                assert c["n_filter_survivors"] == want, (rid, label, name, c["n_filter_survivors"], want)
            if A:
                g = _with_env(env, lambda: ca.search_pipeline(A, params=p, pad_uniform=pad))
                print(json.dumps({"route": rid, "L": label, "set": "A", "n": len(A), "n_pass1": int(g.n_pass1),
                                  "used_fast_filter": int(g.counters["used_fast_filter"])}), flush=True)
                assert g.counters["used_fast_filter"] == want_route
                assert_same_pipeline(g, orc.pipeline(A, params=op))
    assert n_sets > 0
    print("route ok", rid, flush=True)


def _child(rid, env_extra, timeout=600):
    env = dict(os.environ)
    for k in ("CRASS_FF_EXACT", "CRASS_FF_RPL", "CRASS_HINT_RANGE"):
        env.pop(k, None)
    env.update(env_extra)
    code = "from tests.test_gpu_filter_edges import run_route; run_route(%r)" % rid
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert ("route ok " + rid) in r.stdout


@pytest.mark.parametrize("rid", list(ROUTES))
def test_filter_route_edges(rid):
    if ROUTES[rid][4]:
        _child(rid, ROUTES[rid][4])
    else:
        run_route(rid)


S_LENGTHS = (150, 256, 300, 1000, 3000)


@pytest.mark.parametrize("L", S_LENGTHS)
@pytest.mark.parametrize("opts", ["defaults", "d20D40"])
def test_class_switch_reads(opts, L):
    """S: the oracle's record of every read depends on its seed loop leaving the lattice behind a rejected decoy
    (libcrispr.cpp:390).  150 / 256: the lane kernel; 300 / 1 000: the hint filter and the lane or wave kernel; 3 000: the
    long-read path (k_long_light, k_survivor), also without the light walk (CRASS_NO_LIGHT)."""
    import crass_amd as ca
    ca.load()
    p, op = _params(ca, {} if opts == "defaults" else dict(lowDRsize=20, highDRsize=40))
    S, _twins, _tried = E.class_switch_set(E.key(op), L)
    assert len(S) >= 200
    ref = orc.pipeline(S, params=op)
    envs = [{}] + ([{"CRASS_NO_LIGHT": "1"}] if L >= 1000 else [])
    for env in envs:
        g = _with_env(env, lambda: ca.search_pipeline(S, params=p))
        print(json.dumps({"S": opts, "L": L, "env": env, "n": len(S), "n_pass1": int(g.n_pass1), "n_pass2": int(g.n_pass2)}))
        assert_same_pipeline(g, ref)
        assert g.n_pass1 == len(S)


@pytest.mark.parametrize("opts", ["defaults", "d20D40"])
def test_long_read_arrays(opts):
    """A at 3 000 bases (no per-read filter: the long-read path), with the hint kernel in one launch and in three slices"""
    import crass_amd as ca
    ca.load()
    p, op = _params(ca, {} if opts == "defaults" else dict(lowDRsize=20, highDRsize=40))
    A = E.array_set(E.key(op), 3000)
    assert len(A) >= 100
    ref = orc.pipeline(A, params=op)
    for env in ({}, {"CRASS_HINT_PARTS": "3"}, {"CRASS_NO_LIGHT": "1"}):
        g = _with_env(env, lambda: ca.search_pipeline(A, params=p))
        print(json.dumps({"A": opts, "L": 3000, "env": env, "n": len(A), "n_pass1": int(g.n_pass1)}))
        assert_same_pipeline(g, ref)
