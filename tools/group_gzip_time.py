#!/usr/bin/env python3
"""What a plain gzip FASTQ costs on the group's device route (crass_hip_group_set_gzip_on_device), measured, not gated: one run,
medians of --reps (5) with the spread (min .. max), wall seconds around the whole call, on --reads (1 M) synthetic four-line reads
of 100 .. 150 bases compressed by zlib at level 6 as gzip writes them (one member, no flushes), default chunk:
  (a) crass_hip_load_fastx_files on ONE context with crass_hip_set_gzip_on_device: what the group's load is set against;
  (b) the host reader (crass_read_fastx on the file on disk: zlib, one thread);
  (c) the group's load on 1, 2 and 4 CONTEXTS SHARING ONE GPU (local copies), with the distributed inflate alone
      (crass_hip_group_inflate_gzip, host memory to host memory) beside it, its counters and the HIP-event times of its kernels
      on the busiest rank.
Contexts that share one device say nothing about real devices: their kernels, copies and the host are one.
Output: stdout and --out (default profiles/NOTES_r30_group_gzip.txt)."""
import argparse
import os
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch        # (before the library: one HIP runtime in the process, torch's)
import crass_amd as ca

ca.load()
OUT = None


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def wall(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return "%.3f s (%.3f .. %.3f)" % (float(np.median(t)), min(t), max(t))


def make_fastq(n_reads, seed=7):
    rng = np.random.default_rng(seed)
    lens = rng.integers(100, 151, n_reads)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(lens.sum()))]
    quals = np.frombuffer(b"FFFFFFFF:,#F", np.uint8)[rng.integers(0, 12, int(lens.sum()))]
    parts, at = [], 0
    for i, L in enumerate(lens.tolist()):
        parts.append(b"@run7.%d lane=%d/1\n%s\n+\n%s\n" % (i, i % 4, bases[at:at + L].tobytes(), quals[at:at + L].tobytes()))
        at += L
    return b"".join(parts)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "NOTES_r30_group_gzip.txt"))
    a = ap.parse_args()
    OUT = open(a.out, "w") if a.out else None
    text = make_fastq(a.reads)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    zipped = co.compress(text) + co.flush()
    say("device %s; %d reads: text %.3f GB, gzip (level 6, one member) %.3f GB; medians of %d with min .. max" % (
        torch.cuda.get_device_name(0), a.reads, len(text) / 1e9, len(zipped) / 1e9, a.reps))
    with ca.SearchEngine() as e:
        e.set_gzip_on_device(True)
        assert e.load_fastx_files([zipped]).n_reads == a.reads
        say("- (a) one context, gzip on device (crass_hip_load_fastx_files): wall %s" % wall(lambda: e.load_fastx_files([zipped]), a.reps))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fq.gz")
        with open(path, "wb") as f:
            f.write(zipped)
        assert ca.FastxFile(path).n_reads == a.reads
        say("- (b) the host reader (crass_read_fastx): wall %s" % wall(lambda: ca.FastxFile(path), a.reps))
    for n in (1, 2, 4):
        label = "a group of one rank" if n == 1 else "%d contexts sharing one GPU" % n
        with ca.SearchGroup([0] * n, local_copies=n > 1) as g:
            g.set_gzip_on_device(1)
            for r in range(n):
                g.rank_set_stage_timing(r, 1)
            assert g.load_fastx_files([zipped]).n_reads == a.reads
            say("- (c) %s, the load (crass_hip_group_load_fastx_files): wall %s" % (label, wall(lambda: g.load_fastx_files([zipped]), a.reps)))
            assert len(g.inflate_gzip(zipped, out_cap=len(text))) == len(text)
            w = wall(lambda: g.inflate_gzip(zipped, out_cap=len(text)), a.reps)
            c = g.gzip_counters()
            ms = [g.gzip_ms(r) for r in range(n)]
            busiest = max(ms, key=lambda m: sum(m.values()))
            say("      the inflate alone (crass_hip_group_inflate_gzip): wall %s; %d chunks, %d chain elements, %d inflated by a further rank, "
                "%.1f MB uploaded of which %.1f MB more than once; kernels of the busiest rank: %s" % (
                    w, c[1], c[2], c[3], c[4] / 1e6, c[5] / 1e6, ", ".join("%s %.2f ms" % (k, v) for k, v in busiest.items() if k != "tail_windows")))
    say("The contexts of a group here share one device, its copy engines and one host: the rows say what the route costs there, not how")
    say("it scales over real devices, which a one-GPU box cannot measure.")
    if OUT:
        OUT.close()


if __name__ == "__main__":
    main()
