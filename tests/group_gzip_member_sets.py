"""Files and cuts for the tests of the members rule by ranges (tests/test_gzip_members_ranges_host.py,
tests/test_gpu_group_gzip_members.py): the files of tests/gzip_member_sets.py, the cuts of tests/group_gzip_sets.py, and one designed
file whose member boundaries lie on chain-element boundaries and inside elements, with cuts around them.  Everything is seeded;
the designed file's properties are asserted from the plan and the member table, so a zlib that moves them fails loudly."""
import zlib

from tests import group_gzip_sets as ggs
from tests import gzip_sets

CHUNK = ggs.CUT_CHUNK
N_RANGES = ggs.N_RANGES
DESIGNED_CUTS = (0, 70001, 70001, 190003, 333337, 333400, 600011, 845000)
ON_ELEMENTS, INSIDE_ELEMENTS = (190003, 333337, 600011), (70001, 333400, 845000)
TWO_BOUNDARY_ELEMENT = 26


def designed():
    """(file, text): gzip_sets.fastq(201, 1200000) as 8 members cut at DESIGNED_CUTS (one of them empty), every member with a
    Z_BLOCK flush every 3000 text bytes, levels 1 / 6 / 9 in turn"""
    text = gzip_sets.fastq(201, 1200000)
    ends = list(DESIGNED_CUTS[1:]) + [len(text)]
    parts = []
    for m, (a, b) in enumerate(zip(DESIGNED_CUTS, ends)):
        t = text[a:b]
        parts.append(gzip_sets.gz(t, level=(1, 6, 9)[m % 3], flushes=[(p, zlib.Z_BLOCK) for p in range(3000, len(t), 3000)]))
    return b"".join(parts), text


def check_designed(data, text, plan, members):
    """the properties the cuts below rely on, from crass_gzip_inflate_members_host's plan and member table at CHUNK; returns the
    chain's text offsets"""
    off = ggs.chain_offsets(plan)
    assert len(data) == 369478 and len(off) - 1 == 90 and members.n_members == 8, (len(data), len(off) - 1, members.n_members)
    assert [int(x) for x in members.text_off] == list(DESIGNED_CUTS) + [len(text)]
    for b in ON_ELEMENTS:
        assert b in off, b
    for b in INSIDE_ELEMENTS:
        assert b not in off, b
    e = TWO_BOUNDARY_ELEMENT
    assert off[e] == 333337 and off[e] < 333400 < off[e + 1]      # begins a member and holds another boundary
    return off


def member_cuts(off, n_ranges):
    """name -> nominal (n_ranges - 1 text positions) around the designed file's member boundaries, for n_ranges in 2 .. 4"""
    T, k, e = off[-1], n_ranges - 1, TWO_BOUNDARY_ELEMENT
    inside = (off[e] + off[e + 1]) // 2
    out = {"all_at_zero": [0] * k, "all_at_the_end": [T] * k, "all_inside_element_26": [inside + i for i in range(k)],
           "all_between_the_two_boundaries": [333350] * k}
    for b in (70001, 190003):
        for d in (-1, 0, 1):
            out["%d%+d" % (b, d)] = [b + d] * k
        if k >= 2:
            out["around_%d" % b] = [b - 1] + [b + 1] * (k - 1)
    if k >= 2:
        out["boundary_then_inside"] = [190003] + [333350] * (k - 1)
        out["zero_then_the_end"] = [0] + [T] * (k - 1)
    if k >= 3:
        out["three_boundaries"] = [70001, 333337, 600011]
        out["inside_three_elements"] = [70001, 333400, 845000]
    return out


def designed_cuts(off):
    """every designed cut of the designed file: name -> nominal; member_cuts and group_gzip_sets' cuts on the chain"""
    cuts = {"chain_" + k: v for k, v in ggs.boundary_cuts(off).items()}
    for n in (2, 3, 4):
        for k, v in ggs.empty_and_crowded_cuts(off, n).items():
            cuts["chain_%s_%d" % (k, n)] = v
        for k, v in member_cuts(off, n).items():
            cuts["%s_%d" % (k, n)] = v
    return cuts
