"""CRASS_INGEST=device CRASS_DEVICE_GZIP=1 through the complete command line: `crass-hip -g -o DIR --timestamp T --dump-handoff` on a
plain gzip FASTQ (as gzip writes it: one member) — inflated chunk by chunk, parsed and packed on the device — against the same
command without the variables (the indexed reader): the hand-off dump, crass.crispr and every Group_*.fa byte for byte.  Every run
is a fresh child process with its own time limit."""
import gzip
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

STAMP = "01_01_2026_000000"


@pytest.fixture(scope="module")
def cli():
    from crass_amd import build
    return build.build_adapter()


def fastq_with_arrays():
    """12 000 synthetic reads, one in sixteen with a planted array, ragged lengths, as four-line FASTQ"""
    import crass_amd as ca
    ca.load()
    n, L = 12000, 150
    spec = ca.synth_spec(read_len=L, crispr_per_million=60000, n_dr=8)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    recs = []
    for i in range(n):
        s = asc[i * L:(i + 1) * L].tobytes()
        if i % 11 == 0:
            s = s[:70 + (i * 7) % 80]
        recs.append(b"@r%d c%d\n%s\n+\n%s\n" % (i, i % 5, s, bytes(70 + (i + k) % 40 for k in range(len(s)))))
    return b"".join(recs)


def run(cli, args, env_extra, timeout=300):
    env = dict(os.environ)
    env.pop("CRASS_INGEST", None)
    env.pop("CRASS_DEVICE_GZIP", None)
    env.update(env_extra)
    return subprocess.run([cli] + args, capture_output=True, timeout=timeout, env=env)


def test_device_gzip_ingest_writes_the_same_files(cli, tmp_path):
    path = tmp_path / "reads.fastq.gz"
    path.write_bytes(gzip.compress(fastq_with_arrays(), 6))
    assert path.stat().st_size > 2 * 262144                  # (more than one chunk at the default chunk size)
    outs = {}
    for mode, env in (("default", {}), ("device", {"CRASS_INGEST": "device", "CRASS_DEVICE_GZIP": "1", "CRASS_TIMING": "1"})):
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


def test_switch_value_0_keeps_the_decline(cli, tmp_path):
    path = tmp_path / "reads.fastq.gz"
    path.write_bytes(gzip.compress(b"@a\nACGTACGTACGT\n+\nIIIIIIIIIIII\n"))
    out = tmp_path / "out"
    out.mkdir()
    r = run(cli, ["-g", "-o", str(out), "--timestamp", STAMP, str(path)], {"CRASS_INGEST": "device", "CRASS_DEVICE_GZIP": "0"}, timeout=120)
    err = [l for l in r.stderr.decode().split("\n") if "ERROR" in l]
    assert r.returncode != 0 and len(err) == 1 and "reason 10" in err[0], r.stderr.decode()[-2000:]
