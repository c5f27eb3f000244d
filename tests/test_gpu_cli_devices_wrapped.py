"""CRASS_INGEST=devices CRASS_DEVICE_FASTQ=wrapped through the complete command line: `crass-hip -g -o DIR --timestamp T
--dump-handoff` with two contexts on a wrapped FASTQ job of two files — each context cuts its shard at the records reachable from
a file's line 0, parses and packs it on the device, and the handed-on records' sequence, header, comment and quality come back
from the contexts' arenas — against the same command without the variables (the indexed reader): the hand-off dump, crass.crispr
and every Group_*.fa byte for byte.  Without CRASS_DEVICE_FASTQ the same job is the one-line error of before.  Every run is a fresh
child process with its own time limit."""
import os
import subprocess

import pytest

from tests import wrapped_sets

pytestmark = pytest.mark.gpu

STAMP = "01_01_2026_000000"


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


def two_contexts():
    """`--gpus 2 --local-copies` where the box has two devices; on a one-GPU box the two contexts share device 0"""
    import torch
    return ["--gpus", "2", "--local-copies"] if torch.cuda.device_count() >= 2 else ["--devices", "0,0", "--local-copies"]


@pytest.fixture(scope="module")
def wrapped_files():
    """2 x 1 500 synthetic reads, one in sixteen with a planted array, as FASTQ wrapped at 60 columns with comments, quality lines
    that start with '@', blank lines between some records, and names that repeat across the two files"""
    import crass_amd as ca
    ca.load()
    n, L = 3000, 150
    spec = ca.synth_spec(read_len=L, crispr_per_million=60000, n_dr=8)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    parts = []
    for i in range(n):
        s = asc[i * L:(i + 1) * L].tobytes()
        if i % 11 == 0:
            s = s[:70 + i % 80]
        q = bytes(64 + (k + i) % 40 if k % 60 else 64 for k in range(len(s)))      # (every quality line starts with '@')
        name = b"r%d" % (i if i % 3 else (7 * i + 1) % n)
        parts.append(wrapped_sets.wfq(name + b" c%d" % (i % 7), s, q, w=60, after=(b"",) if i % 13 == 0 else ()))
    return b"".join(parts[:n // 2]) + b"\n", b"".join(parts[n // 2:])


def run(cli, args, env_extra, timeout=300):
    env = dict(os.environ)
    for k in ("CRASS_INGEST", "CRASS_DEVICE_FASTQ", "CRASS_SHARD_MARGIN"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([cli] + args, capture_output=True, timeout=timeout, env=env)


def write(tmp_path, files):
    paths = []
    for k, data in enumerate(files):
        p = tmp_path / ("w%d.fq" % k)
        p.write_bytes(data)
        paths.append(str(p))
    return paths


def test_wrapped_devices_ingest_writes_the_same_files(cli, wrapped_files, tmp_path):
    paths = write(tmp_path, wrapped_files)
    outs = {}
    more = two_contexts()                                # (the same device arguments in both runs: crass.crispr records the command line)
    for mode, env in (("default", {}), ("devices", {"CRASS_INGEST": "devices", "CRASS_DEVICE_FASTQ": "wrapped", "CRASS_TIMING": "1"})):
        d = tmp_path / mode
        d.mkdir()
        r = run(cli, ["-g", "-o", str(d), "--timestamp", STAMP, "--dump-handoff"] + more + paths, env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if mode == "devices":
            assert "crass_hip_group_load_fastx_files" in r.stderr.decode()
        outs[mode] = {f: open(d / f, "rb").read().replace(str(d).encode(), b"DIR") for f in sorted(os.listdir(d))}
    want, got = outs["default"], outs["devices"]
    assert want.keys() == got.keys()
    compared = [f for f in want if f in ("crass_hip_handoff.tsv", "crass.crispr") or f.startswith("Group_")]
    assert "crass_hip_handoff.tsv" in compared and "crass.crispr" in compared and any(f.startswith("Group_") for f in compared)
    for f in compared:
        assert got[f] == want[f], f
    rows = [l.split(b"\t") for l in got["crass_hip_handoff.tsv"].split(b"\n") if l.startswith(b"R\t")]
    assert len(rows) > 50 and any(len(r) > 9 and len(r[9]) == len(r[7]) > 60 and r[9][:1] == b"@" for r in rows)


def one_error_line(r, needle):
    err = [l for l in r.stderr.decode().split("\n") if "ERROR" in l]
    assert r.returncode != 0 and len(err) == 1 and err[0].startswith("crass [ERROR]: ") and needle in err[0], r.stderr.decode()[-2000:]
    return err[0]


def test_without_the_variable_the_error_is_as_before(cli, wrapped_files, tmp_path):
    import crass_amd as ca
    paths = write(tmp_path, wrapped_files)
    four = ca.fastx_files_scan_host(list(wrapped_files))
    assert not four.accepted and four.decline_file == 0
    lines = []
    for env in ({"CRASS_INGEST": "devices"}, {"CRASS_INGEST": "devices", "CRASS_DEVICE_FASTQ": "four-line"}):
        out = tmp_path / ("out%d" % len(lines))
        out.mkdir()
        r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP] + two_contexts() + paths, env, timeout=120)
        line = one_error_line(r, paths[0])
        assert ("(reason %d)" % four.decline_reason) in line and ("at byte %d" % four.decline_pos) in line and "CRASS_INGEST=devices cannot take" in line
        lines.append((line, r.returncode))
    assert lines[0] == lines[1]


def test_a_wrapped_decline_and_a_wrong_value_are_one_line_errors(cli, wrapped_files, tmp_path):
    bad, reason, pos = wrapped_sets.declines(4096)["empty_then_at_last"]
    paths = write(tmp_path, [wrapped_files[1], bad])
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP] + two_contexts() + paths, {"CRASS_INGEST": "devices", "CRASS_DEVICE_FASTQ": "wrapped"}, timeout=120)
    line = one_error_line(r, paths[1])
    assert "(reason 12)" in line and ("at byte %d" % pos) in line and "an empty sequence" in line
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP] + two_contexts() + paths, {"CRASS_INGEST": "devices", "CRASS_DEVICE_FASTQ": "multi"}, timeout=120)
    one_error_line(r, "CRASS_DEVICE_FASTQ=multi")
