"""CRASS_INGEST=device CRASS_DEVICE_GZIP=2 through the complete command line: `crass-hip -g -o DIR --timestamp T --dump-handoff` on
a `cat` of two gzip'd FASTQ files with planted arrays — a plain gzip file of two members, inflated chunk by chunk in members mode,
parsed and packed on the device — against the same command without the variables (the indexed reader): the hand-off dump,
crass.crispr and every Group_*.fa byte for byte.  With CRASS_DEVICE_GZIP=1 the run fails as it did before the value 2 existed.
Every run is a fresh child process with its own time limit."""
import gzip
import os

import pytest

from tests.test_gpu_cli_gzip_ingest import STAMP, fastq_with_arrays, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


@pytest.fixture(scope="module")
def two_members():
    text = fastq_with_arrays()
    cut = text.index(b"\n@r6000 ") + 1                      # (the first file ends on a record boundary, as files do)
    return gzip.compress(text[:cut], 6) + gzip.compress(text[cut:], 9)


def test_device_gzip_members_ingest_writes_the_same_files(cli, two_members, tmp_path):
    path = tmp_path / "all.fastq.gz"
    path.write_bytes(two_members)
    assert path.stat().st_size > 2 * 262144                  # (more than one chunk at the default chunk size)
    outs = {}
    for mode, env in (("default", {}), ("device", {"CRASS_INGEST": "device", "CRASS_DEVICE_GZIP": "2", "CRASS_TIMING": "1"})):
        d = tmp_path / mode
        d.mkdir()
        r = run(cli, ["-g", "-o", str(d), "--timestamp", STAMP, "--dump-handoff", str(path)], env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if mode == "device":
            assert "crass_hip_load_fastx_files" in r.stderr.decode()
        outs[mode] = {f: open(d / f, "rb").read().replace(str(d).encode(), b"DIR") for f in sorted(os.listdir(d))}
    want, got = outs["default"], outs["device"]
    assert want.keys() == got.keys()
    compared = [f for f in want if f in ("crass_hip_handoff.tsv", "crass.crispr") or f.startswith("Group_")]
    assert "crass_hip_handoff.tsv" in compared and "crass.crispr" in compared and any(f.startswith("Group_") for f in compared)
    for f in compared:
        assert got[f] == want[f], f
    rows = [l.split(b"\t") for l in got["crass_hip_handoff.tsv"].split(b"\n") if l.startswith(b"R\t")]
    assert len(rows) > 100


def test_switch_value_1_keeps_the_decline(cli, two_members, tmp_path):
    path = tmp_path / "all.fastq.gz"
    path.write_bytes(two_members)
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP, str(path)], {"CRASS_INGEST": "device", "CRASS_DEVICE_GZIP": "1"}, timeout=120)
    err = [l for l in r.stderr.decode().split("\n") if "ERROR" in l]
    assert r.returncode != 0 and len(err) == 1 and "reason 13" in err[0], r.stderr.decode()[-2000:]
