"""Designed FASTA inputs for the header ids and header lines computed on the device (test_gpu_header_ids.py): names chosen
for what a name table can get wrong.  Generated data only; everything is deterministic.  At most 200 records each."""
import random

from tests.fastx_sets import acgt, fa

LONG = 3 * 4096 + 5              # a name of three scan tiles and a bit
EDGE_LENGTHS = (252, 255, 256, 257, 258, 259, 260, 261, 264, 511, 512, 513)      # around where names go from a lane to a wave


def _name(rng, n):
    return bytes(rng.choices(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_/.:#|>@+-", k=n))


def designed():
    """name -> bytes, inside the regular class of the record scan"""
    rng = random.Random("header_sets:designed")
    d = {}
    seq = lambda: acgt(rng, rng.randint(1, 90))

    # ---- long names, prefixes, empty names, bytes >= 128 and NUL ----
    long_name = _name(rng, LONG)
    other_last = long_name[:-1] + (b"Q" if long_name[-1:] != b"Q" else b"R")
    recs = [fa(long_name, seq(), 60), fa(b"short", seq()), fa(long_name + b" second copy, with a comment", seq()),
            fa(other_last, seq()), fa(long_name[:LONG - 7], seq()), fa(long_name[:3], seq()), fa(long_name[:3], seq()),
            fa(long_name[:3 * 4096], seq()), fa(other_last + b"\tc", seq())]
    recs += [fa(b"", seq()), fa(b" comment only", seq()), fa(b"", b""), fa(b"\tx", seq())]      # the empty name, four times
    for nm in (b"n\x80m", b"n\x81m", b"n\x00m", b"n\x01m", b"n\x80m", b"n\x00m", b"n", b"n\x00", b"n\x00", b"n\xff", b"\x00", b"\x00\x00", b"\x00"):
        recs.append(fa(nm, seq()))
    for nm in (b"x", b"x ", b"x\ty", b"x\x0by", b"x\x0cy", b"x\ry", b"xy", b"x\x1fy", b"x\x1fy z", b"x\x0ey"):      # isspace() cuts; 0x0E, 0x1F do not
        recs.append(fa(nm, seq()))
    # ---- names around the lane / wave threshold: each twice, and once with another last byte ----
    for n in EDGE_LENGTHS:
        nm = _name(rng, n)
        recs += [fa(nm, seq()), fa(nm[:-1] + (b"!" if nm[-1:] != b"!" else b"?"), seq()), fa(nm + b" again", seq())]
    # ---- one name at all 16 byte alignments: a filler record in front moves it ----
    data = b"".join(recs)
    for t in range(16):
        pad = (t - (len(data) + len(b">p%02d\n\n" % t))) % 16
        data += fa(b"p%02d" % t, b"A" * (pad + 16))
        assert len(data) % 16 == t
        data += fa(b"same-name-everywhere/1", seq())
    # ---- the long name once more, as the last line without its '\n': a name that ends with the input ----
    data += b">" + long_name
    d["designed"] = data
    assert data.count(b"\n>") + 1 <= 200

    # a short repeated name that ends with the input, behind names that share its dwords
    d["tail_dupe"] = b">dupe\nAC\n>dup\nA\n>dupe1\nC\n>dupe comment\nG\n>dupe"
    return d


def header_lines(data, rec_pos):
    """the header lines of an accepted input from its record positions: behind the header character, up to the '\\n' or the end"""
    out = []
    for r in range(len(rec_pos) - 1):
        a = int(rec_pos[r]) + 1
        e = data.find(b"\n", a)
        out.append(data[a:e if e >= 0 else len(data)])
    return out
