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
--members N (N >= 1) writes the same reads as N concatenated members cut at even text positions and takes them in MEMBERS mode:
(a) is the single context's members load, (c) the group with mode 2 and crass_hip_group_inflate_gzip_members, with the members
counters (files, members, CRC pieces, exported windows without a reference); with N = 1 the group's mode 1 is timed beside it.
Output: stdout and --out (default profiles/NOTES_r30_group_gzip.txt; with --members profiles/NOTES_r31_group_gzip_members_N.txt)."""
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
    ap.add_argument("--members", type=int, default=0, help="N >= 1: the reads as N concatenated members, taken in members mode")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mem = a.members >= 1
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                             "NOTES_r31_group_gzip_members_%d.txt" % a.members if mem else "NOTES_r30_group_gzip.txt")
    OUT = open(a.out, "w") if a.out else None
    text = make_fastq(a.reads)
    n_mem = max(a.members, 1)
    zipped = b""
    for k in range(n_mem):
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        zipped += co.compress(text[len(text) * k // n_mem:len(text) * (k + 1) // n_mem]) + co.flush()
    say("device %s; %d reads: text %.3f GB, gzip (level 6, %d member%s%s) %.3f GB; medians of %d with min .. max" % (
        torch.cuda.get_device_name(0), a.reads, len(text) / 1e9, n_mem, "" if n_mem == 1 else "s", ", members mode" if mem else "", len(zipped) / 1e9, a.reps))
    with ca.SearchEngine() as e:
        e.set_gzip_on_device(True, members=mem)
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
            g.set_gzip_on_device(2 if mem else 1)
            for r in range(n):
                g.rank_set_stage_timing(r, 1)
            assert g.load_fastx_files([zipped]).n_reads == a.reads
            say("- (c) %s, the load (crass_hip_group_load_fastx_files): wall %s" % (label, wall(lambda: g.load_fastx_files([zipped]), a.reps)))
            inflate = g.inflate_gzip_members if mem else g.inflate_gzip
            assert len(inflate(zipped, out_cap=len(text))) == len(text)
            w = wall(lambda: inflate(zipped, out_cap=len(text)), a.reps)
            c = g.gzip_counters()
            ms = [g.gzip_ms(r) for r in range(n)]
            busiest = max(ms, key=lambda m: sum(m.values()))
            say("      the inflate alone (crass_hip_group_inflate_gzip%s): wall %s; %d chunks, %d chain elements, %d inflated by a further rank, "
                "%.1f MB uploaded of which %.1f MB more than once; kernels of the busiest rank: %s" % (
                    "_members" if mem else "", w, c[1], c[2], c[3], c[4] / 1e6, c[5] / 1e6, ", ".join("%s %.2f ms" % (k, v) for k, v in busiest.items() if k != "tail_windows")
                    + (", member_crc %.2f ms" % max(g.gzip_members_ms(r)["member_crc"] for r in range(n)) if mem else "")))
            if mem:
                say("      members counters: %d file, %d members, %d CRC pieces, %d exported windows without a reference" % g.gzip_members_counters())
            if mem and n_mem == 1:
                g.set_gzip_on_device(1)
                say("      the same group with mode 1, the load: wall %s" % wall(lambda: g.load_fastx_files([zipped]), a.reps))
    say("The contexts of a group here share one device, its copy engines and one host: the rows say what the route costs there, not how")
    say("it scales over real devices, which a one-GPU box cannot measure.")
    if OUT:
        OUT.close()


if __name__ == "__main__":
    main()
