"""CRASS_INGEST=devices through the complete command line: `crass-hip -g -o DIR --timestamp T --dump-handoff` on two-file inputs —
the files cut into record-aligned shards, one per context, each parsed, inflated and packed on the device beside the others
(crass_hip_group_load_fastx_files), the handed-on records' sequence, header, comment and quality fetched back from the ranks —
against the same command without the variable (the indexed reader): the hand-off dump, crass.crispr and every Group_*.fa byte
for byte, with two contexts on one device and with one.  A declined input is a one-line error with the position in the whole
file.  Every run is a fresh child process with its own time limit."""
import os

import pytest

from tests.test_gpu_cli_device_ingest import STAMP, fq, inputs, one_error_line, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


@pytest.fixture(scope="module")
def records():
    """6 000 synthetic reads, one in sixteen with a planted array: ragged lengths, N reads; names repeat inside a file and across
    the two files (the pattern of tests/test_gpu_cli_device_ingest.py's records)"""
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
        out.append((b"r%d" % (i if i % 97 else (i // 2) % 3000 + 3000 * (i % 2)), s))
    return out


@pytest.fixture(scope="module")
def default_outputs(cli, records, tmp_path_factory):
    """the default reader's outputs for an input kind and the same device arguments (crass.crispr records the command line)"""
    made = {}

    def get(kind, more):
        if kind not in made:
            base = tmp_path_factory.mktemp("in_" + kind)
            made[kind] = (base, inputs(kind, records, base))
        base, paths = made[kind]
        d = base / ("default" + "".join(more).replace(",", ""))
        d.mkdir()
        r = run(cli, ["-g", "-o", str(d), "--timestamp", STAMP, "--dump-handoff"] + more + paths, {})
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return paths, {f: open(d / f, "rb").read().replace(str(d).encode(), b"DIR") for f in sorted(os.listdir(d))}
    return get


def two_contexts():
    """`--gpus 2 --local-copies` where the box has two devices; on a one-GPU box --gpus 2 names a device that is not there, so the two
    contexts share device 0, as in tests/test_gpu_adapter.py"""
    import torch
    return ["--gpus", "2", "--local-copies"] if torch.cuda.device_count() >= 2 else ["--devices", "0,0", "--local-copies"]


@pytest.mark.parametrize("gpus", [2, 1])
@pytest.mark.parametrize("kind", ["plain", "bgzf", "fasta_fastq"])
def test_devices_ingest_writes_the_same_files(cli, default_outputs, tmp_path, kind, gpus):
    more = two_contexts() if gpus == 2 else ["--gpus", "1"]
    paths, want = default_outputs(kind, more)
    d = tmp_path / "devices"
    d.mkdir()
    r = run(cli, ["-g", "-o", str(d), "--timestamp", STAMP, "--dump-handoff"] + more + paths, {"CRASS_INGEST": "devices", "CRASS_TIMING": "1"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert "devices ingest" in r.stderr.decode() and "crass_hip_group_load_fastx_files" in r.stderr.decode()
    got = {f: open(d / f, "rb").read().replace(str(d).encode(), b"DIR") for f in sorted(os.listdir(d))}
    assert want.keys() == got.keys()
    compared = [f for f in want if f in ("crass_hip_handoff.tsv", "crass.crispr") or f.startswith("Group_")]
    assert "crass_hip_handoff.tsv" in compared and "crass.crispr" in compared and any(f.startswith("Group_") for f in compared)
    for f in compared:
        assert got[f] == want[f], (kind, gpus, f)
    rows = [l.split(b"\t") for l in got["crass_hip_handoff.tsv"].split(b"\n") if l.startswith(b"R\t")]
    assert len(rows) > 100 and {r[3] for r in rows} == {b"0", b"1"}


def test_an_irregular_fastq_in_the_second_ranks_part_is_an_error_with_its_position(cli, records, tmp_path):
    good = fq(records[:40])
    tail = fq(records[40:45])
    (tmp_path / "a.fq").write_bytes(good + b"@x\nACGT\n+\nII\n" + tail)      # (beyond the middle: the second rank's part)
    assert len(good) > len(tail) + 20
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP] + two_contexts() + [str(tmp_path / "a.fq")], {"CRASS_INGEST": "devices"}, timeout=120)
    line = one_error_line(r, str(tmp_path / "a.fq"))
    assert "CRASS_INGEST=devices" in line and "(reason 8)" in line and ("at byte %d" % (len(good) + len(b"@x\nACGT\n+\n"))) in line
