"""CRASS_INGEST=device through the complete command line: `crass-hip -g -o DIR --timestamp T --dump-handoff` on two-file inputs — the
files parsed, inflated and packed on the device as one read set, the handed-on records' sequence, header, comment and quality
fetched back from the device — against the same command without the variable (the indexed reader): the hand-off dump, crass.crispr
and every Group_*.fa byte for byte.  A declined input and more than one device are one-line errors.  Every run is a fresh child
process with its own time limit."""
import os
import subprocess

import pytest

from tests import files_sets

pytestmark = pytest.mark.gpu

STAMP = "01_01_2026_000000"


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


@pytest.fixture(scope="module")
def records():
    """6 000 synthetic reads, one in sixteen with a planted array: ragged lengths, N reads; (name, sequence) pairs in which names
    repeat inside the set, so that they repeat inside a file and across the two files"""
    import crass_amd as ca
    import numpy as np
    ca.load()
    n, L = 6000, 150
    spec = ca.synth_spec(read_len=L, crispr_per_million=60000, n_dr=8)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    rng = np.random.default_rng(15)
    out = []
    for i in range(n):
        s = asc[i * L:(i + 1) * L].tobytes()
        if i % 11 == 0:
            s = s[:int(rng.integers(70, L))]
        if i % 501 == 0:
            s = s[:40] + b"N" + s[41:]
        out.append((b"r%d" % (i if i % 97 else (i // 2) % 3000 + 3000 * (i % 2)), s))      # (every 97th: a name of the other half too)
    return out


def fa(recs):
    return b"".join(b">" + nm + b"\n" + s + b"\n" for nm, s in recs)


def fq(recs):
    return b"".join(b"@" + nm + b" c" + nm + b"\n" + s + b"\n+\n" + bytes(70 + (k + i) % 40 for i in range(len(s))) + b"\n" for k, (nm, s) in enumerate(recs))


def inputs(kind, recs, d):
    h = len(recs) // 2
    if kind == "plain":
        files = {"a.fq": fq(recs[:h]), "b.fq": fq(recs[h:])}
    elif kind == "bgzf":
        files = {"a.fa.gz": files_sets.bgzf_sets.bgzf(fa(recs[:h])), "b.fa.gz": files_sets.bgzf_sets.bgzf(fa(recs[h:]), block=20000)}
    elif kind == "fasta_fastq":
        files = {"a.fa": fa(recs[:h]), "b.fq.gz": files_sets.bgzf_sets.bgzf(fq(recs[h:]))}
    paths = []
    for name, data in files.items():
        (d / name).write_bytes(data)
        paths.append(str(d / name))
    return paths


def run(cli, args, env_extra, timeout=300):
    env = dict(os.environ)
    env.pop("CRASS_INGEST", None)
    env.update(env_extra)
    return subprocess.run([cli] + args, capture_output=True, timeout=timeout, env=env)


@pytest.mark.parametrize("kind", ["plain", "bgzf", "fasta_fastq"])
def test_device_ingest_writes_the_same_files(cli, records, tmp_path, kind):
    paths = inputs(kind, records, tmp_path)
    outs = {}
    for mode, env in (("default", {}), ("device", {"CRASS_INGEST": "device", "CRASS_TIMING": "1"})):
        d = tmp_path / mode
        d.mkdir()
        r = run(cli, ["-g", "-o", str(d), "--timestamp", STAMP, "--dump-handoff"] + paths, env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if mode == "device":
            assert "device ingest" in r.stderr.decode() and "crass_hip_load_fastx_files" in r.stderr.decode()
        outs[mode] = {f: open(d / f, "rb").read().replace(str(d).encode(), b"DIR") for f in sorted(os.listdir(d))}
    want, got = outs["default"], outs["device"]
    assert want.keys() == got.keys()
    compared = [f for f in want if f in ("crass_hip_handoff.tsv", "crass.crispr") or f.startswith("Group_")]
    assert "crass_hip_handoff.tsv" in compared and "crass.crispr" in compared and any(f.startswith("Group_") for f in compared)
    for f in compared:
        assert got[f] == want[f], (kind, f)
    # the hand-off is not trivial: records with a quality string (FASTQ) and without one (FASTA), comments, both orientations
    rows = [l.split(b"\t") for l in got["crass_hip_handoff.tsv"].split(b"\n") if l.startswith(b"R\t")]
    assert len(rows) > 100 and {r[3] for r in rows} == {b"0", b"1"}
    if kind != "bgzf":
        assert any(r[5] == b"0" and len(r) > 9 and len(r[9]) == len(r[7]) > 0 and r[8] for r in rows)
    if kind != "plain":
        assert any(r[5] == b"1" and (len(r) < 10 or not r[9]) for r in rows)


def one_error_line(r, needle):
    err = [l for l in r.stderr.decode().split("\n") if "ERROR" in l]
    assert r.returncode != 0 and len(err) == 1 and err[0].startswith("crass [ERROR]: ") and needle in err[0], r.stderr.decode()[-2000:]
    return err[0]


def test_a_plain_gzip_input_is_an_error(cli, records, tmp_path):
    import gzip
    (tmp_path / "a.fa").write_bytes(fa(records[:50]))
    (tmp_path / "b.fa.gz").write_bytes(gzip.compress(fa(records[50:100])))
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP, str(tmp_path / "a.fa"), str(tmp_path / "b.fa.gz")], {"CRASS_INGEST": "device"}, timeout=120)
    line = one_error_line(r, str(tmp_path / "b.fa.gz"))
    assert "reason 10" in line and "at byte 0" in line


def test_an_irregular_fastq_is_an_error_with_its_position(cli, records, tmp_path):
    good = fq(records[:10])
    (tmp_path / "a.fq").write_bytes(good + b"@x\nACGT\n+\nII\n")
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP, str(tmp_path / "a.fq")], {"CRASS_INGEST": "device"}, timeout=120)
    line = one_error_line(r, str(tmp_path / "a.fq"))
    assert "(reason 8)" in line and ("at byte %d" % (len(good) + len(b"@x\nACGT\n+\n"))) in line


def test_more_than_one_device_is_an_error(cli, records, tmp_path):
    (tmp_path / "a.fa").write_bytes(fa(records[:50]))
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP, "--gpus", "2", "--local-copies", str(tmp_path / "a.fa")], {"CRASS_INGEST": "device"}, timeout=120)
    one_error_line(r, "one device")
