"""The window argument behind pass 2's anchor probe, on the CPU: for the (KL, A) the engine selects for a lowDRsize — KL bases
per key, a window every A bases (dm_anchor_shape, crass_amd/csrc/engine_internal.h) — every occurrence of a pattern of at least
lowDRsize bases contains the read's aligned KL-base window at ceil_A(offset), and that window is one of the pattern's A keys.
The rule: a pair is admissible iff KL + A - 1 <= lowDRsize, KL in {16, 12}, A in {8, 4}.  No compute entry point is called."""
import ctypes as C
import random

import pytest

KEY_BASES = (16, 12)        # a 32-bit or a 24-bit key
ALIGNS = (8, 4)             # halfword or byte positions of the packed words


@pytest.fixture(scope="module")
def shape():
    import crass_amd
    from crass_amd import build
    build.build()
    lib = C.CDLL(crass_amd.LIB_PATH)
    lib.crassi_anchor_shape.restype = C.c_int
    lib.crassi_anchor_shape.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]

    def f(low):
        kl, a = C.c_uint32(0), C.c_uint32(0)
        ok = lib.crassi_anchor_shape(low, C.byref(kl), C.byref(a))
        return (kl.value, a.value) if ok else None
    return f


def admissible(low):
    return [(kl, a) for kl in KEY_BASES for a in ALIGNS if kl + a - 1 <= low]


def test_the_table_of_key_shapes(shape):
    for low in range(23, 65):
        assert shape(low) == (16, 8)
    for low in range(19, 23):
        assert shape(low) == (16, 4)
    for low in range(15, 19):
        assert shape(low) == (12, 4)
    for low in range(0, 15):
        assert shape(low) is None


def test_every_selected_shape_is_admissible_and_14_has_none(shape):
    for low in range(15, 65):
        assert shape(low) in admissible(low), low
    assert admissible(14) == [] and admissible(11) == []
    assert admissible(15) == [(12, 4)]                 # 12 + 4 - 1 = 15: the only pair, hence the floor


@pytest.mark.parametrize("low", [15, 16, 17, 18, 19, 22, 23, 30])
def test_aligned_window_lies_inside_every_occurrence(shape, low):
    kl, a = shape(low)
    rng = random.Random(low)
    for plen in sorted(set([low, low + 1, low + 6, 33, 64]) | {rng.randint(low, 64) for _ in range(4)}):
        if plen < low:
            continue
        pat = bytes(rng.choice(b"ACGT") for _ in range(plen))
        keys = {pat[r:r + kl] for r in range(a)}
        L = 150
        for o in range(0, L - plen + 1):
            read = bytearray(rng.choice(b"ACGT") for _ in range(L))
            read[o:o + plen] = pat
            w = -(-o // a) * a                          # ceil_A(o)
            assert o <= w <= o + a - 1
            assert w + kl <= o + plen, (low, plen, o)   # the window lies inside the occurrence
            assert w + kl <= L                          # ... so it is one of the windows the probe visits: (L - KL) // A of them
            assert w // a <= (L - kl) // a
            assert bytes(read[w:w + kl]) == pat[w - o:w - o + kl]
            assert bytes(read[w:w + kl]) in keys


def test_one_base_less_breaks_the_argument(shape):
    """the bound is tight: a pattern of KL + A - 2 bases at offset 1 (mod A) does not contain its aligned window"""
    for low in (15, 19, 23):
        kl, a = shape(low)
        plen, o = kl + a - 2, 1
        w = -(-o // a) * a
        assert w + kl > o + plen
