"""bench.py's own options: the plain run against --full, and --dump-outputs (the last timed step's results, which must equal
the oracle's on the same synthetic reads)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    crass_amd.load()
    return crass_amd


def _oracle(ca, n, L=150):
    spec = ca.synth_spec(read_len=L, n_dr=50, gc_classes=0, crispr_per_million=10000, array_min_repeats=0, array_max_repeats=0)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    return orc.pipeline((asc, np.arange(0, (n + 1) * L, L, dtype=np.uint64)))


def test_output_arrays_layout(ca):
    """every table row is the result's own record / token / pattern; the sample is fixed and shrinks to the byte limit"""
    import bench
    res = _oracle(ca, 300000)
    a = bench.output_arrays(res)
    assert all(v.dtype == np.float64 for v in a.values())
    s = a["summary"]
    assert list(s[:5]) == [res.n_pass1, res.n_pass2, res.n_tokens, res.n_groups, res.n_patterns] and res.n_pass1 > 1000
    assert s[5] == float(res.rec_read.sum()) and s[7] == float(res.rec_token.sum())
    recs, ss = a["records"], a["records_ss"]
    assert len(recs) == res.n_pass1 + res.n_pass2
    for row, pos in zip(recs, ss):
        k = int(row[0])
        assert list(row[1:6]) == [res.rec_read[k], res.rec_lowlexi[k], res.rec_token[k], res.rec_replen[k], res.rec_nss[k]]
        assert row[6] == (1 if k < res.n_pass1 else 2)
        want = res.ss(k)
        assert list(pos[:len(want)]) == want and np.all(pos[len(want):] == -1)
    for row in a["tokens"]:
        t = res.tokens[int(row[0])]
        assert row[1] == len(t) and bytes(row[2:2 + len(t)].astype(np.uint8)) == t and not row[2 + len(t):].any()
    assert [(int(g), int(t)) for g, t in a["groups"]] == [(g, t) for g, grp in enumerate(res.groups) for t in grp]
    for row in a["patterns"]:
        p = res.patterns[int(row[0])]
        assert row[1] == res.pat_group[int(row[0])] and row[2] == len(p) and bytes(row[3:3 + len(p)].astype(np.uint8)) == p
    small = bench.output_arrays(res, limit=100000)
    assert sum(v.nbytes for v in small.values()) <= 100000 and 0 < len(small["records"]) < len(recs)
    assert np.array_equal(small["records"], bench.output_arrays(res, limit=100000)["records"])
    assert np.all(np.diff(small["records"][:, 0]) > 0)


@pytest.mark.parametrize("opt", [["--check"], ["--cpu-sample", "1000"], ["--single-shots", "2"], ["--e2e-reads", "1000"]])
def test_extras_need_full(opt):
    """options that only act on the extra measurements refuse to run without --full, before anything starts"""
    r = subprocess.run([sys.executable, BENCH, "--steps", "1"] + opt, capture_output=True, timeout=120)
    assert r.returncode == 2 and b"--full" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_oracle_result(ca, tmp_path):
    """a plain run: the headline fields, none of the --full extras, and outputs equal to the oracle's on the same reads"""
    n = 300000
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--total-reads", str(n), "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = json.loads([line for line in r.stdout.decode().splitlines() if line.startswith("{")][-1])
    assert d["unit"] == "reads/s" and d["higher_is_better"] is True and d["dtype"] == "u8" and d["steps"] == 3
    assert d["ms_per_step"] > 0 and abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    for key in ("roofline", "cpu_baseline", "single_shot_ms", "abi_fetch_ms", "e2e", "parity_checked"):
        assert key not in d
    import bench
    want = bench.output_arrays(_oracle(ca, n))
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    for k, v in want.items():
        got = np.load(out / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, v), k
