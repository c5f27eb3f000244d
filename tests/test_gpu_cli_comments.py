"""A mixed input through the complete command line: two files in which every third header line carries a comment, so that two
records in three are handed the comment of an earlier record of their file, as kseq's buffer hands it on.  `crass-hip -g -o DIR
--timestamp T --dump-handoff` with CRASS_INGEST=device, and with CRASS_INGEST=devices on two contexts, against the same command
without the variable (the host readers): the hand-off dump, crass.crispr and every Group_*.fa byte for byte; the dump holds at
least 20 records whose comment is not on their own header line.  Every run is a fresh child process with its own time limit."""
import os

import pytest

from tests.test_gpu_cli_device_ingest import STAMP, run
from tests.test_gpu_cli_devices_ingest import two_contexts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


def comment_of(name):
    return b"c" + name + b" x"


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """6 000 synthetic reads with unique names, one in sixteen with a planted array, as a FASTA and a FASTQ file; record i of a
    file has a comment of its own iff i % 3 == 1 — so record 0 of each file is in front of its file's first comment.  Returns
    (paths, {name: (the comment on its own line or None, the comment kseq hands it or None)})"""
    import crass_amd as ca
    ca.load()
    n, L = 6000, 150
    spec = ca.synth_spec(read_len=L, crispr_per_million=60000, n_dr=8)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    recs = [(b"r%d" % i, asc[i * L:(i + 1) * L].tobytes()) for i in range(n)]
    d = tmp_path_factory.mktemp("mixed")
    what, texts = {}, []
    for half, fastq in ((recs[:n // 2], False), (recs[n // 2:], True)):
        out, carried = [], None
        for i, (nm, s) in enumerate(half):
            own = comment_of(nm) if i % 3 == 1 else None
            carried = own if own is not None else carried
            what[nm] = (own, carried)
            head = nm + (b" " + own if own is not None else b"")
            out.append(b"@" + head + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" if fastq else b">" + head + b"\n" + s + b"\n")
        texts.append(b"".join(out))
    (d / "a.fa").write_bytes(texts[0])
    (d / "b.fq").write_bytes(texts[1])
    return [str(d / "a.fa"), str(d / "b.fq")], what


def outputs(cli, d, more, paths, env):
    d.mkdir()
    r = run(cli, ["-g", "-o", str(d), "--timestamp", STAMP, "--dump-handoff"] + more + paths, env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stderr.decode(), {f: open(d / f, "rb").read().replace(str(d).encode(), b"DIR") for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("route", ["device", "devices"])
def test_a_mixed_input_writes_the_same_files(cli, job, tmp_path, route):
    paths, what = job
    more = two_contexts() if route == "devices" else []
    _, want = outputs(cli, tmp_path / "default", more, paths, {})
    err, got = outputs(cli, tmp_path / route, more, paths, {"CRASS_INGEST": route, "CRASS_TIMING": "1"})
    assert ("devices ingest" if route == "devices" else "device ingest") in err
    assert want.keys() == got.keys()
    compared = [f for f in want if f in ("crass_hip_handoff.tsv", "crass.crispr") or f.startswith("Group_")]
    assert "crass_hip_handoff.tsv" in compared and "crass.crispr" in compared and any(f.startswith("Group_") for f in compared)
    # the dump is not trivial: records that are handed an earlier record's comment, records with their own, records with none
    rows = [l.split(b"\t") for l in want["crass_hip_handoff.tsv"].split(b"\n") if l.startswith(b"R\t")]
    assert len(rows) > 100
    handed_on = [r for r in rows if r[8] and what[r[2]][0] is None]
    assert len(handed_on) >= 20 and any(r[8] and what[r[2]][0] == r[8] for r in rows)
    for r in rows:
        assert r[8] == (what[r[2]][1] or b""), r[2]
    for f in compared:
        assert got[f] == want[f], (route, f)
