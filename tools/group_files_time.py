#!/usr/bin/env python3
"""What the files route of a group costs (crass_hip_group_load_fastx_files), measured, not gated: one run, medians of --reps (3).

  (1) k_fx_cut_probe's HIP-event time per GB of text against a device-to-device copy of the same bytes (hipMemcpy between two
      torch tensors, HIP events) — the probe is a stream, one byte read per byte;
  (2) a group of ONE rank against crass_hip_load_fastx_files on the same files: two files of --reads / 2 synthetic 150 bp reads
      each (default 2 x 2 M, as the files-load notes), plain FASTQ and BGZF, wall seconds;
  (3) groups of 2 and of 4 CONTEXTS SHARING ONE GPU (local copies) on the same files.  This is not scaling over devices: the
      contexts' kernels and copies share one device, one bus and one host.  What scaling over real devices gives cannot be measured
      on a one-GPU box.
Output: stdout and profiles/NOTES_r21.md (--out)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch        # (before the library: one HIP runtime in the process, torch's)
import crass_amd as ca
from tools.load_files_time import bgzf, fastq_bytes

ca.load()
OUT = None


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def med(v):
    return float(np.median(v))


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return med(out)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "NOTES_r21.md"))
    a = ap.parse_args()
    OUT = open(a.out, "w")
    say("# Device ingest across the ranks of a group: measured once, medians of %d\n" % a.reps)
    half = a.reads // 2
    texts = [fastq_bytes(0, half, a.len), fastq_bytes(half, a.reads - half, a.len)]
    say("Two files, %d + %d reads of %d bp, %.3f GB of text.\n" % (half, a.reads - half, a.len, sum(len(t) for t in texts) / 1e9))
    # (1) the probe against a copy
    say("## k_fx_cut_probe against a device-to-device copy\n")
    gb = len(texts[0]) / 1e9
    with ca.SearchEngine() as e:
        src = torch.from_numpy(np.frombuffer(texts[0], np.uint8).copy()).cuda()
        dst = torch.empty_like(src)
        e.set_stage_timing(1)
        e.cut_probe_device(int(src.data_ptr()), src.numel(), True)
        probe = []
        for _ in range(a.reps):
            e.cut_probe_device(int(src.data_ptr()) + 1, src.numel() - 1, False)
            probe.append(e.last_cut_probe_ms())
    copy = []
    dst.copy_(src)
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        copy.append(e0.elapsed_time(e1))
    say("- probe: %.3f ms for %.3f GB = %.3f ms per GB (%.0f GB/s read)" % (med(probe), gb, med(probe) / gb, gb / (med(probe) / 1e3)))
    say("- copy:  %.3f ms for %.3f GB = %.3f ms per GB (%.0f GB/s read + as much written)\n" % (med(copy), gb, med(copy) / gb, gb / (med(copy) / 1e3)))
    del src, dst
    # (2), (3) the loads
    say("## The group's files load against the single context's\n")
    sets = {"plain": [np.frombuffer(t, np.uint8) for t in texts], "bgzf": [np.frombuffer(bgzf(t), np.uint8) for t in texts]}
    with ca.SearchEngine() as e:
        for kind, bufs in sets.items():
            e.load_fastx_files(bufs)
            say("- %-5s crass_hip_load_fastx_files (one context): wall %.3f s" % (kind, wall(lambda: e.load_fastx_files(bufs), a.reps)))
    for n, label in ((1, "a group of one rank"), (2, "2 contexts sharing one GPU"), (4, "4 contexts sharing one GPU")):
        with ca.SearchGroup([0] * n, local_copies=n > 1) as g:
            for kind, bufs in sets.items():
                g.load_fastx_files(bufs)
                say("- %-5s crass_hip_group_load_fastx_files, %s: wall %.3f s" % (kind, label, wall(lambda: g.load_fastx_files(bufs), a.reps)))
    say("\nThe contexts of the last two rows share one device, its copy engines and one host: the rows say what the route costs there,")
    say("not how it scales.  Scaling over real devices cannot be measured on a one-GPU box.")
    OUT.close()


if __name__ == "__main__":
    main()
