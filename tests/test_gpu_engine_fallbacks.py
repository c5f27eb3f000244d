"""Every site where a device merge that gave up ends in the host merge (CRASS_DM_INJECT_FAIL raises a software status word in
the merge's state, no kernel fault): the non-speculative and the speculative site of crass_hip_recruit, a context's second
step with a merge queued from the seed scan, a global merge (the concatenated list copied back from the device) through a
group and through crass_hip_merge_distinct, and crass_hip_get_merge before pass 2.  Each result equals the oracle's and the
counters show the fall-back."""
import os

import numpy as np
import pytest

from crass_amd.engine import PipelineResult
from tests import orc
from tests.parity import assert_same_pipeline
from tests.test_gpu_parity import synth_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def seqs(ca):
    return synth_reads(ca, 20000, read_len=150, n_dr=10, crispr_per_million=30000)


@pytest.fixture(scope="module")
def ref(seqs):
    return orc.pipeline(seqs)


def assert_fell_back(cnt):
    assert cnt["n_merge_fallbacks"] >= 1 and cnt["last_fallback_bits"] != 0 and cnt["used_device_merge"] == 0


def with_env(fn, **env):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def test_non_speculative_site(ca, seqs, ref):
    got = with_env(lambda: ca.search_pipeline(seqs), CRASS_DM_INJECT_FAIL="1", CRASS_NO_SPECULATION="1")
    assert_fell_back(got.counters)
    assert_same_pipeline(got, ref)


def test_speculative_site_on_a_second_step(ca, seqs, ref):
    """the second call of a context runs with learnt bounds and a merge queued from the seed scan"""
    def two_steps():
        eng = ca.SearchEngine()
        try:
            return ca.search_pipeline(seqs, engine=eng), ca.search_pipeline(seqs, engine=eng)
        finally:
            eng.close()
    a, b = with_env(two_steps, CRASS_DM_INJECT_FAIL="1")
    for got in (a, b):
        assert_fell_back(got.counters)
        assert_same_pipeline(got, ref)
    assert b.counters["n_merge_fallbacks"] >= 2


@pytest.mark.parametrize("fused", [True, False])
def test_global_merge_of_a_group(ca, seqs, ref, fused):
    grp = with_env(lambda: ca.search_pipeline_group(seqs, [0, 0], local_copies=True, fused=fused), CRASS_DM_INJECT_FAIL="1")
    assert len(grp.counters) == 2
    for cnt in grp.counters:
        assert_fell_back(cnt)
    assert_same_pipeline(grp, ref)


def test_global_merge_through_merge_distinct(ca, seqs, ref):
    """a world of one: the context's own distinct list is the concatenation (crass_hip_merge_distinct)"""
    def run():
        eng = ca.SearchEngine()
        packed = ca.PackedReads(seqs)
        try:
            eng.load_reads(packed, None)
            cand = eng.seed_scan()
            chars, lens, _ = eng.distinct()
            eng.merge_distinct(np.array(chars), np.array(lens), 0, fetch=False)
            rec = eng.recruit()
            res = PipelineResult(cand, eng.merge_view(), rec, cand.max_read_len)
            res.counters = eng.counters()
            return res
        finally:
            eng.close()
            packed.close()
    got = with_env(run, CRASS_DM_INJECT_FAIL="1")
    assert_fell_back(got.counters)
    assert_same_pipeline(got, ref)


def test_merge_view_before_pass_2(ca, seqs, ref):
    """crass_hip_get_merge on a merge that gave up, nothing fetched before it: the view is the host merge's"""
    def run():
        eng = ca.SearchEngine()
        packed = ca.PackedReads(seqs)
        try:
            eng.load_reads(packed, None)
            eng.seed_scan(fetch=False)
            eng.merge(fetch=False)
            m = eng.merge_view()
            view = (m.tokens, m.groups, m.patterns, m.pat_group.tolist(), m.cand_token.tolist(), m.next_free_gid)
            cand = eng.candidates()
            rec = eng.recruit()
            res = PipelineResult(cand, eng.merge_view(), rec, cand.max_read_len)
            res.counters = eng.counters()
            return view, res
        finally:
            eng.close()
            packed.close()
    view, got = with_env(run, CRASS_DM_INJECT_FAIL="1")
    host_view, host = with_env(run, CRASS_HOST_MERGE="1")
    assert host.counters["n_merge_fallbacks"] == 0 and host.counters["used_device_merge"] == 0
    assert view == host_view
    assert_fell_back(got.counters)
    assert_same_pipeline(got, ref)
