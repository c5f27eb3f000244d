"""CRASS_INGEST=devices CRASS_DEVICE_GZIP=2 through the complete command line: `crass-hip -g -o DIR --timestamp T` with two contexts
on a `cat` of two plain gzip FASTQ files — the group's devices inflate the file together in members mode
(crass_hip_group_set_gzip_on_device with CRASS_GZIP_ON_DEVICE_MEMBERS), then cut it into shards — against the same command on the
text: crass.crispr and every Group_*.fa byte for byte.  With CRASS_DEVICE_GZIP=1 the input fails as before (further members: reason
13).  Every run is a fresh child process with its own time limit."""
import gzip

import pytest

from tests.test_gpu_cli_device_ingest import STAMP, fq, one_error_line, run
from tests.test_gpu_cli_devices_gzip import outputs
from tests.test_gpu_cli_devices_ingest import records, two_contexts      # noqa: F401  (records: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


def cat_of_two(text):
    """the text as `cat a.gz b.gz`: the first member ends in the middle of a record"""
    at = len(text) // 2 + 7
    return gzip.compress(text[:at], 6) + gzip.compress(text[at:], 9)


def test_a_cat_of_two_gzip_files_writes_the_same_files_as_its_text(cli, records, tmp_path):
    text = fq(records)
    got = {}
    # (the same file name in two directories: crass.crispr records the command line)
    for mode, data, env in (("text", text, {}), ("zipped", cat_of_two(text), {"CRASS_DEVICE_GZIP": "2"})):
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


def test_with_the_variable_at_1_further_members_are_the_error_they_were(cli, records, tmp_path):
    (tmp_path / "reads.fq.gz").write_bytes(cat_of_two(fq(records[:200])))
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP] + two_contexts() + [str(tmp_path / "reads.fq.gz")],
            {"CRASS_INGEST": "devices", "CRASS_DEVICE_GZIP": "1"}, timeout=120)
    line = one_error_line(r, str(tmp_path / "reads.fq.gz"))
    assert "reason 13" in line
