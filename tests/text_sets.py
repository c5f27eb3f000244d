"""Seeded read sets as sequence text, shared by the device packer's tests (test_load_text_abi.py, test_gpu_load_text.py)."""
import random

import numpy as np

SPECIAL_LENGTHS = [0, 1, 15, 16, 17, 32, 48, 160, 1600, 4992, 5000]

# name -> builder(ca, rng) -> list of bytes
LAYOUT_SETS = ["uniform150", "synth100k", "trimmed", "ragged", "exc_ends", "all_exc", "odd_bytes", "n0", "n1", "n63", "n64", "n65",
               "n1500", "empty_reads", "long_ragged"]


def _acgt(rng, n):
    return bytes(rng.choices(b"ACGT", k=n))


def concat(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy() if seqs else np.zeros(0, np.uint8)
    return buf, off


def synth_text(ca, n, read_len=150, seed=7):
    """the repository's synthetic metagenome (crass_synth_packed) as ASCII reads"""
    words = ca.synth_packed(ca.synth_spec(read_len=read_len, seed=seed), 0, n)
    asc = ca.unpack_ascii(words, (read_len + 15) // 16, read_len, n)
    return [asc[i * read_len:(i + 1) * read_len].tobytes() for i in range(n)]


def with_n(rng, s, k=1):
    b = bytearray(s)
    for _ in range(k):
        if b:
            b[rng.randrange(len(b))] = ord("N")
    return bytes(b)


def make(ca, name):
    rng = random.Random("text_sets:" + name)
    if name == "uniform150":
        return [_acgt(rng, 150) for _ in range(3000)]
    if name == "synth100k":
        return synth_text(ca, 100000)
    if name == "trimmed":                                # 64 .. 151 bases: padding rule 2 applies
        s = [_acgt(rng, rng.randint(64, 151)) for _ in range(4000)]
        return [with_n(rng, x) if i % 97 == 5 else x for i, x in enumerate(s)]
    if name == "ragged":                                 # 1 .. 5 000 bases, the special lengths, exact multiples of 16
        lens = SPECIAL_LENGTHS + [16 * rng.randint(1, 300) for _ in range(40)] + [rng.randint(1, 5000) for _ in range(600)] + [rng.randint(1, 40) for _ in range(300)]
        rng.shuffle(lens)
        s = [_acgt(rng, n) for n in lens]
        return [with_n(rng, x, 2) if i % 41 == 7 else x for i, x in enumerate(s)]
    if name == "exc_ends":                               # the first and the last read are exception reads
        s = [_acgt(rng, rng.randint(30, 400)) for _ in range(700)]
        s[0] = with_n(rng, s[0]); s[-1] = s[-1][:-1] + b"n"
        return s
    if name == "all_exc":
        return [with_n(rng, _acgt(rng, 150), rng.randint(1, 5)) for _ in range(2500)]
    if name == "odd_bytes":                              # lower case, N, 0x00, 0xFF
        out = []
        for i in range(1200):
            L = rng.randint(1, 300)
            kind = i % 6
            if kind == 0:
                out.append(bytes(rng.choices(b"acgt", k=L)))
            elif kind == 1:
                out.append(b"N" * L)
            elif kind == 2:
                out.append(bytes(rng.choices(b"ACGT\x00", k=L)))
            elif kind == 3:
                out.append(bytes(rng.choices(b"ACGT\xff", k=L)))
            elif kind == 4:
                out.append(bytes(rng.choices(b"ACGTacgtNU\x00\xff", k=L)))
            else:
                out.append(_acgt(rng, L))
        return out
    if name in ("n0", "n1", "n63", "n64", "n65", "n1500"):      # 1 500 reads of 150 bases: not a multiple of a block's reads
        n = int(name[1:])
        return [_acgt(rng, 150) if i % 9 else with_n(rng, _acgt(rng, 150)) for i in range(n)]
    if name == "empty_reads":                            # empty reads at both ends and in runs
        lens = [0, 0, 0, 5, 0, 16, 0, 0, 33, 0] * 30 + [0, 0]
        return [_acgt(rng, n) for n in lens]
    if name == "long_ragged":                            # 300 .. 5 000 bases with N reads
        s = [_acgt(rng, rng.randint(300, 5000)) for _ in range(400)]
        return [with_n(rng, x, 3) if i % 23 == 3 else x for i, x in enumerate(s)]
    raise KeyError(name)
