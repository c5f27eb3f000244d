"""CRASS_INGEST=devices CRASS_DEVICE_GZIP=1 through the complete command line: `crass-hip -g -o DIR --timestamp T` with two contexts
on a plain gzip FASTQ — the group's devices inflate the file together (crass_hip_group_set_gzip_on_device), then cut it into
shards — against the same command on the inflated file: crass.crispr and every Group_*.fa byte for byte.  Without the variable
the input is the error it was.  Every run is a fresh child process with its own time limit."""
import gzip
import os

import pytest

from tests.test_gpu_cli_device_ingest import STAMP, fq, one_error_line, run
from tests.test_gpu_cli_devices_ingest import records, two_contexts      # noqa: F401  (records: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


def outputs(d, replace):
    out = {}
    for f in sorted(os.listdir(d)):
        b = open(d / f, "rb").read()
        for old, new in replace:
            b = b.replace(str(old).encode(), new)
        out[f] = b
    return out


def test_a_plain_gzip_fastq_writes_the_same_files_as_its_text(cli, records, tmp_path):
    text = fq(records)
    got = {}
    # (the same file name in two directories: crass.crispr records the command line)
    for mode, data, env in (("text", text, {}), ("zipped", gzip.compress(text, 6), {"CRASS_DEVICE_GZIP": "1"})):
        base = tmp_path / mode
        (base / "out").mkdir(parents=True)
        (base / "reads.fq.gz").write_bytes(data)
        env = dict(env, CRASS_INGEST="devices", CRASS_TIMING="1")
        r = run(cli, ["-g", "-o", str(base / "out"), "--timestamp", STAMP] + two_contexts() + [str(base / "reads.fq.gz")], env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert "devices ingest" in r.stderr.decode()
        got[mode] = outputs(base / "out", [(base, b"DIR")])
    assert got["text"].keys() == got["zipped"].keys()
    compared = [f for f in got["text"] if f == "crass.crispr" or f.startswith("Group_")]
    assert "crass.crispr" in compared and any(f.startswith("Group_") for f in compared)
    for f in compared:
        assert got["zipped"][f] == got["text"][f], f


def test_without_the_variable_a_plain_gzip_input_is_the_error_it_was(cli, records, tmp_path):
    (tmp_path / "reads.fq.gz").write_bytes(gzip.compress(fq(records[:200])))
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP] + two_contexts() + [str(tmp_path / "reads.fq.gz")], {"CRASS_INGEST": "devices"}, timeout=120)
    line = one_error_line(r, str(tmp_path / "reads.fq.gz"))
    assert "reason 10" in line and "at byte 0" in line
