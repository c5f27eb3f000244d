#!/usr/bin/env python3
"""What it costs to get TWO input files (paired-end style) resident as one packed read set: the indexed host reader against the
device route for several files (crass_hip_load_fastx_files), and the command line end to end with either.

Synthetic 150 bp reads (--reads N in all, default 4 M; half in each file) as four-line FASTQ, written once to a scratch directory
as plain text and as BGZF (members of 60 000 bytes of text, zlib level 1).  Median of --reps (3), in one process and in this
order, wall and CPU seconds each, for the plain pair and for the BGZF pair:
  (a) crass_index_fastx_files + crass_hip_load_reads       the indexed reader (maps / inflates, parses and packs on the host)
  (b) crass_hip_load_fastx_files                           the files' bytes go up as they are; inflate, scan, pack and header ids
                                                           on the device (the files are read into memory before the clock starts
                                                           for (b) and are mapped inside it for (a): the page cache holds both)
and crass_hip_last_inflate_ms / _scan_ms / _pack_ms / _header_ids_ms of (b) (HIP events, timing level 1).
Then `crass-hip -g -o DIR` on the same pairs, a fresh process per run, wall seconds of the parent's clock:
  (c) default reader (the index)          (d) CRASS_INGEST=device
--no-cli leaves (c) / (d) out.  Output: stdout and profiles/load_files_mi355x.txt (--out)."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import crass_amd as ca
from crass_amd import build

ca.load()
OUT = None


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def med(v):
    return float(np.median(v))


def timed(fn, reps):
    wall, cpu = [], []
    for _ in range(reps):
        w0, c0 = time.perf_counter(), time.process_time()
        fn()
        wall.append(time.perf_counter() - w0)
        cpu.append(time.process_time() - c0)
    return med(wall), med(cpu)


def fastq_bytes(first, n, L):
    """n synthetic reads from read `first` on as a four-line FASTQ, built with numpy: '@' + an 8-digit name, the read, '+', 'I' * L"""
    spec = ca.synth_spec(read_len=L, crispr_per_million=10000)
    asc = ca.unpack_ascii(ca.synth_packed(spec, first, n), (L + 15) // 16, L, n).reshape(n, L)
    rec = np.empty((n, 1 + 8 + 1 + L + 3 + L + 1), np.uint8)
    rec[:, 0] = ord("@")
    idx = np.arange(first, first + n, dtype=np.int64)
    for d in range(8):
        rec[:, 8 - d] = ord("0") + (idx // 10 ** d) % 10
    rec[:, 9] = 10
    rec[:, 10:10 + L] = asc
    rec[:, 10 + L:13 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 13 + L:13 + 2 * L] = ord("I")
    rec[:, 13 + 2 * L] = 10
    return rec.tobytes()


def bgzf(text, block=60000, level=1):
    out = []
    for i in list(range(0, len(text), block)) + [None]:
        c = b"" if i is None else text[i:i + block]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        d = co.compress(c) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 12 + 6 + len(d) + 8 - 1) + d +
                   struct.pack("<II", zlib.crc32(c) & 0xFFFFFFFF, len(c)))
    return b"".join(out)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "load_files_mi355x.txt"))
    a = ap.parse_args()
    OUT = open(a.out, "w")
    half = a.reads // 2
    with tempfile.TemporaryDirectory() as td:
        texts = [fastq_bytes(0, half, a.len), fastq_bytes(half, a.reads - half, a.len)]
        pairs = {}
        for kind, make, ext in (("plain", lambda t: t, ".fq"), ("bgzf", bgzf, ".fq.gz")):
            paths = []
            for k, t in enumerate(texts):
                p = os.path.join(td, "reads_%d%s" % (k + 1, ext))
                with open(p, "wb") as f:
                    f.write(make(t))
                paths.append(p)
            pairs[kind] = paths
        say("two files, %d + %d reads of %d bp, %.3f GB of text; plain %.3f GB, BGZF %.3f GB on disk" % (
            half, a.reads - half, a.len, sum(len(t) for t in texts) / 1e9, sum(os.path.getsize(p) for p in pairs["plain"]) / 1e9,
            sum(os.path.getsize(p) for p in pairs["bgzf"]) / 1e9))
        del texts
        with ca.SearchEngine() as e:
            e.set_stage_timing(1)
            for kind, paths in pairs.items():
                def host_route():
                    ix = ca.FastxIndex(paths)
                    e.load_reads(ix)
                    ix.close()
                bufs = [np.fromfile(p, dtype=np.uint8) for p in paths]
                host_route()
                e.load_fastx_files(bufs)                      # (first calls: allocations, code objects)
                wa, ca_ = timed(host_route, a.reps)
                wb, cb = timed(lambda: e.load_fastx_files(bufs), a.reps)
                say("%-5s (a) crass_index_fastx_files + crass_hip_load_reads  wall %.3f s  CPU %.3f s" % (kind, wa, ca_))
                say("%-5s (b) crass_hip_load_fastx_files                      wall %.3f s  CPU %.3f s   (a) / (b) = %.2f" % (kind, wb, cb, wa / wb if wb else 0.0))
                say("%-5s     kernels of the last (b): inflate %.3f ms, scan %.3f ms, pack %.3f ms, header ids %.3f ms" % (
                    kind, e.last_inflate_ms(), e.last_scan_ms(), e.last_pack_ms(), e.last_header_ids_ms()[0]))
                del bufs
        if not a.no_cli:
            cli = build.build_adapter()
            for kind, paths in pairs.items():
                for tag, env in (("(c) default reader", {}), ("(d) CRASS_INGEST=device", {"CRASS_INGEST": "device"})):
                    walls = []
                    for rep in range(a.reps):
                        d = os.path.join(td, "out_%s_%s_%d" % (kind, tag[1], rep))
                        os.mkdir(d)
                        full = dict(os.environ)
                        full.pop("CRASS_INGEST", None)
                        full.update(env)
                        w0 = time.perf_counter()
                        r = subprocess.run([cli, "-g", "-o", d] + paths, capture_output=True, env=full, timeout=1200)      # (a fresh child process per run)
                        walls.append(time.perf_counter() - w0)
                        if r.returncode != 0:
                            say("%-5s %s FAILED (exit %d): %s" % (kind, tag, r.returncode, r.stderr.decode()[-300:]))
                            break
                    say("%-5s %-24s crass-hip end to end  wall %.3f s (median of %d)" % (kind, tag, med(walls), len(walls)))
    OUT.close()


if __name__ == "__main__":
    main()
