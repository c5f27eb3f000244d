"""The pass-1 seed filter with two shifts folded per minimum (k_filter_fast_pairs): a LOOSE scan on 14 of a seed's 16 bits
through v_bitop3_b32 / v_pk_minimum3_f16, then the EXACT scan of k_filter_fast_impl on the loose positives.  Its hit mask and
hints must be k_filter_fast_impl's bit for bit, so nothing behind the filter may differ: CRASS_FF_EXACT=1 keeps the exact kernel
everywhere and is the other side of the comparisons here.  The switch and CRASS_FF_RPL are read once per process, so every run
is a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (100, 101, 125, 126, 150, 151, 250, 251)
SIZES = ((1 << 22) - 1, (1 << 22) + 1000)          # below the switch to four rows per lane (one kernel for both runs), and above
M14 = 0x3FFF                                        # what the loose scan keeps of a seed halfword


# ---- CPU: the property "no false negative" rests on ----
def test_loose_predicate_is_implied_by_the_exact_one():
    """For every xor halfword x: the masked halfword x & 0x3FFF, read as f16, is finite and not negative (no NaN, no Inf, no
    sign: minimum3 cannot lose it to a NaN and orders it like the unsigned integer), it is +0 for x = 0 (an exact hit is a loose
    hit), and +0 only for x in {0, 0x4000, 0x8000, 0xC000} (the loose hit is "the first seven bases match")."""
    x = np.arange(65536, dtype=np.uint32)
    masked = (x & M14).astype(np.uint16)
    f = masked.view(np.float16)
    assert np.all(np.isfinite(f)) and not np.any(np.signbit(f))
    assert masked[0] == 0 and f[0] == 0
    assert sorted(x[masked == 0].tolist()) == [0, 0x4000, 0x8000, 0xC000]
    # as f16 the masked halfwords order exactly like the integers, denormals (0x0001 .. 0x03FF) included
    order = np.arange(M14 + 1, dtype=np.uint16).view(np.float16).astype(np.float64)
    assert np.all(np.diff(order) > 0)
    # so the three-input f16 minimum of masked halfwords is their unsigned minimum; in particular it is 0 iff one of them is
    rng = np.random.default_rng(5)
    t = rng.integers(0, M14 + 1, size=(200000, 3), dtype=np.uint16)
    t[:1000, 0] = 0
    t[1000:3000, 1] = rng.integers(1, 0x400, 2000, dtype=np.uint16)       # denormals
    t[3000:5000, 2] = rng.integers(0x3C00, 0x4000, 2000, dtype=np.uint16)  # exponent 0b01111
    assert np.array_equal(t.view(np.float16).min(axis=1).view(np.uint16), t.min(axis=1))


# ---- GPU: the two kernels give the same pass 1 ----
def _child(code, env_extra, timeout):
    env = dict(os.environ)
    env.pop("CRASS_FF_EXACT", None)
    env.pop("CRASS_FF_RPL", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


_SWEEP = r"""
import hashlib, json, sys
import numpy as np
import crass_amd as ca
ca.load()
lengths, sizes = json.loads(sys.argv[1]), json.loads(sys.argv[2])
for L in lengths:
    spec = ca.synth_spec(read_len=L, crispr_per_million=20000)
    words = ca.synth_packed(spec, 0, max(sizes))
    for n in sizes:
        with ca.SearchEngine() as eng:
            eng.load_packed_uniform(words, n, L)
            c = eng.seed_scan()
            cnt = eng.counters()
            h = hashlib.sha256()
            for a in (c.read_idx, c.low_lexi, c.repeat_len, c.n_ss, c.ss_off, c.ss_pool, c.dr_len, c.dr_chars):
                h.update(np.ascontiguousarray(a).tobytes())
            print(json.dumps({"L": L, "n": n, "n_pass1": int(c.n), "records": h.hexdigest(),
                              "counters": {k: int(cnt[k]) for k in ("n_reads", "n_exceptions", "n_filter_survivors", "n_pass1_found", "used_fast_filter")}}), flush=True)
"""


@pytest.mark.gpu
def test_pairs_and_exact_kernels_give_the_same_pass1():
    """Uniform lengths with a compile-time clamp, sizes on both sides of the four-rows-per-lane switch: counters
    (n_filter_survivors is the hit mask's population count) and every pass-1 record with and without CRASS_FF_EXACT=1."""
    args = [json.dumps(list(LENGTHS)), json.dumps(list(SIZES))]
    runs = []
    for extra in ({}, {"CRASS_FF_EXACT": "1"}):
        env = dict(os.environ)
        env.pop("CRASS_FF_EXACT", None)
        env.pop("CRASS_FF_RPL", None)
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", _SWEEP] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")])
    pairs, exact = runs
    assert len(pairs) == len(exact) == len(LENGTHS) * len(SIZES)
    for a, b in zip(pairs, exact):
        print(a)
        assert a == b
        assert a["counters"]["used_fast_filter"] == 1 and 0 < a["counters"]["n_filter_survivors"] < a["n"] and a["n_pass1"] > 0


# ---- GPU: adversarial reads against a model of the exact predicate and the oracle ----
L_ADV = 150
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def exact_filter_model(seqs, L=L_ADV, d0=49, d1=97):
    """The filter's contract, restated: read r survives iff for some lattice seed j = 8h <= L - d0 - 9 the 8-mer at j re-occurs
    at j + d for a d in d0 .. min(d1, L - 9 - 16 (h // 2)); a non-ACGT byte counts as 'A' and so does everything past the read's
    end (the zero padding of the packed row)."""
    n = len(seqs)
    a = np.frombuffer(b"".join(seqs), np.uint8).reshape(n, L)
    codes = np.zeros((n, L + 128), np.uint8)
    for byte, code in _CODE.items():
        codes[:, :L][a == byte] = code
    hit = np.zeros(n, bool)
    for h in range((L - d0 - 9) // 8 + 1):
        seed = codes[:, 8 * h:8 * h + 8]
        for d in range(d0, min(d1, L - 9 - 16 * (h // 2)) + 1):
            hit |= np.all(seed == codes[:, 8 * h + d:8 * h + d + 8], axis=1)
    return hit


def adversarial_reads(seed=11):
    """(reads, kinds): 150 bp reads whose planted copy of one lattice seed is exact, or differs from it in chosen bases only."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    flip3 = {65: 84, 84: 65, 67: 71, 71: 67}          # code xor 3
    flip1 = {65: 67, 67: 65, 71: 84, 84: 71}          # code xor 1
    n = 6 * 1024 + 389                                 # (not a multiple of a block's 1 024 reads)
    reads = letters[rng.integers(0, 4, size=(n, L_ADV))]
    kinds = []
    for i in range(n):
        blk = i // 1024
        h = int(rng.integers(0, 12))
        d = int(rng.integers(49, min(97, L_ADV - 9 - 16 * (h // 2), L_ADV - 8 - 8 * h) + 1))     # (the whole copy inside the read)
        if blk == 0:
            kind = "b7"                                # a whole block of loose-only reads: every lane queues, the queue is full
        elif blk == 1:
            kind, h, d = ("same", "b7")[i & 1], 11, 49 + (i % 6)        # the last seed word (h = 11: word 5, high half)
        elif blk == 2:
            kind = ("den0", "den4", "exp15", "b7")[i & 3]
        elif blk == 3:
            kind = ("same", "b7", "none", "none")[i & 3]
        else:
            kind = ("none", "none", "none", "same", "b7", "den0", "exp15", "none")[i & 7]
        kinds.append(kind)
        if kind == "none":
            continue
        copy = reads[i, 8 * h:8 * h + 8].copy()
        if kind == "b7":                               # only the eighth base differs: xor halfword 0x4000 / 0x8000 / 0xC000
            copy[7] = letters[(int(np.where(letters == copy[7])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == "den0":                           # xor halfword 0x0001: the smallest f16 denormal
            copy[0] = flip1[int(copy[0])]
        elif kind == "den4":                           # xor halfword 0x03FF: the largest
            for b in range(5):
                copy[b] = flip3[int(copy[b])]
        elif kind == "exp15":                          # xor halfword 0x3C00: exponent 0b01111, mantissa 0 (f16 1.0)
            copy[5], copy[6] = flip3[int(copy[5])], flip3[int(copy[6])]
        reads[i, 8 * h + d:8 * h + d + 8] = copy
    # exception reads: an N outside the planted seed and its copy, and one inside a seed (it packs as 'A')
    for i in range(3 * 1024 + 5, n, 97):
        reads[i, 148] = ord("N")
    for i in range(3 * 1024 + 50, n, 211):
        reads[i, int(rng.integers(0, 90))] = ord("N")
    return [reads[i].tobytes() for i in range(n)], kinds


_ADV = r"""
import numpy as np
import crass_amd as ca
from tests import orc
from tests.parity import assert_same_pipeline
from tests.test_gpu_filter_pairs import adversarial_reads, exact_filter_model
ca.load()
seqs, kinds = adversarial_reads()
model = exact_filter_model(seqs)
kinds = np.array(kinds)
print("reads", len(seqs), "model survivors", int(model.sum()), {k: (int((kinds == k).sum()), int(model[kinds == k].sum())) for k in sorted(set(kinds.tolist()))}, flush=True)
assert model[kinds == "same"].all()                                     # an exact copy survives
assert (kinds == "b7").sum() >= 1000 and model[kinds == "b7"].mean() < 0.05     # loose-only reads do not (but for chance repeats)
gpu = ca.search_pipeline(seqs, device=0)
print("gpu counters", gpu.counters, flush=True)
assert gpu.counters["used_fast_filter"] == 1 and gpu.counters["n_exceptions"] > 0
assert gpu.counters["n_filter_survivors"] == int(model.sum()), (gpu.counters["n_filter_survivors"], int(model.sum()))
assert_same_pipeline(gpu, orc.pipeline(seqs))
print("adversarial ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["pairs", "exact"])
def test_adversarial_reads_survive_exactly_as_the_model_says(exact):
    """Reads built to separate the loose test from the exact one (see adversarial_reads), through the four-rows-per-lane form
    (CRASS_FF_RPL=4: k_filter_fast_pairs, or k_filter_fast_impl with CRASS_FF_EXACT=1).  The survivor count is the model's
    (exact_filter_model, written from the filter's contract, not from either kernel) and the pipeline's records are the
    oracle's."""
    out = _child(_ADV, dict({"CRASS_FF_RPL": "4"}, **({"CRASS_FF_EXACT": "1"} if exact else {})), 900)
    print(out[-3000:])
    assert "adversarial ok" in out
