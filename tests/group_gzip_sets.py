"""Cuts for the tests of a gzip inflate by ranges (tests/test_gzip_ranges_host.py, tests/test_gpu_group_gzip.py): from the plan of a
file (crass_gzip_plan) the text offsets of its chain elements, and nominal cuts designed around them — on an element boundary,
one byte to either side of it, inside the first and the last element, cuts that leave a range without text, and cuts that put
several ranges inside one element.  The files themselves are tests/gzip_sets.py's."""
import numpy as np

LINK_END, LINK_NONE = 0xFFFFFFFF, 0xFFFFFFFC
N_RANGES = (1, 2, 3, 4, 7)
CUT_CHUNK = 4096


def chain_offsets(plan):
    """text offsets [n_chain + 1] of the chain elements of a GzipPlan of an accepted file"""
    off, k = [0], 0
    while True:
        off.append(off[-1] + int(plan.text_len[k]))
        if int(plan.link[k]) == LINK_END:
            break
        assert int(plan.link[k]) < LINK_NONE
        k = int(plan.link[k])
    assert len(off) == plan.n_chain + 1
    return off


def boundary_cuts(off):
    """name -> nominal (n_ranges - 1 text positions) around the chain's element boundaries; the chain has at least 4 elements with text"""
    T, n = off[-1], len(off) - 1
    assert n >= 4 and off[1] > 2 and T - off[n - 1] > 2
    mid = off[n // 2]                                      # a boundary in the middle
    assert off[n // 2 - 1] < mid - 1 and mid + 1 < off[n // 2 + 1]
    first, last = off[1] // 2, (off[n - 1] + T) // 2     # inside the first and the last element
    return {
        "on_a_boundary": [mid],
        "one_before": [mid - 1],
        "one_behind": [mid + 1],
        "inside_the_first": [first],
        "inside_the_last": [last],
        "both_sides_of_a_boundary": [mid - 1, mid + 1],
        "boundaries_in_a_row": [off[n // 2 - 1], mid, off[n // 2 + 1]],
        "first_and_last": [first, last],
        "first_boundary_and_last": [off[1], off[n - 1]],
    }


def empty_and_crowded_cuts(off, n_ranges):
    """name -> nominal for n_ranges in 2 .. 4: ranges without text (on a boundary: no element; at the text's ends) and
    every inner cut inside ONE element (all the ranges hold it)"""
    T, n = off[-1], len(off) - 1
    mid = off[n // 2]
    inside = (off[n // 2] + off[n // 2 + 1]) // 2
    k = n_ranges - 1
    return {
        "all_at_a_boundary": [mid] * k,
        "all_at_zero": [0] * k,
        "all_at_the_end": [T] * k,
        "all_at_one_byte": [inside] * k,
        "crowded_in_one_element": [inside + i for i in range(k)],
        "zero_then_the_end": ([0] + [T] * (k - 1)) if k > 1 else [0],
    }


def as_u64(nominal):
    return np.asarray(nominal, dtype=np.uint64)
