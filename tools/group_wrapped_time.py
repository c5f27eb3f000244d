#!/usr/bin/env python3
"""What wrapped FASTQ costs in a group's files load (crass_hip_group_set_fastq_class), measured, not gated: one run, medians of
--reps (3), wall seconds around the whole call, on --reads (2 M) synthetic 150 bp reads wrapped at 60 columns and on their
four-line form:
  (1) crass_hip_load_fastx_files with class 1 on ONE context, the wrapped file: what the group's load is set against;
  (2) the group's load with class 1 on 1, 2 and 4 CONTEXTS SHARING ONE GPU (local copies), the wrapped file: two attempts, the
      second cut by the chain.  Per load: the HIP-event time of the cut kernels (k_fw_summary .. k_fw_cut_jump) summed over the ranks and
      the largest rank's, the chain look-ups and the margin doublings (crass_hip_group_load_counters);
  (3) the same groups on the four-line form with class 1 (one attempt, the same kernels as class 0) against class 0.
Contexts that share one device say nothing about real devices: their kernels, copies and the host are one.
Output: stdout and --out (default profiles/NOTES_r29_group_wrapped.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch        # (before the library: one HIP runtime in the process, torch's)
import crass_amd as ca
from tools.wrapped_scan_time import make_files

ca.load()
OUT = None


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "NOTES_r29_group_wrapped.txt"))
    a = ap.parse_args()
    OUT = open(a.out, "w") if a.out else None
    four, wrapped = make_files(a.reads)
    say("device %s; %d reads of 150 bases: four-line %.3f GB, wrapped at 60 columns %.3f GB; medians of %d" % (
        torch.cuda.get_device_name(0), a.reads, len(four) / 1e9, len(wrapped) / 1e9, a.reps))
    with ca.SearchEngine() as e:
        e.set_fastq_class(1)
        assert e.load_fastx_files([wrapped]).n_reads == a.reads and e.last_scan_classes() == (0, 1)
        say("- one context, class 1, wrapped (crass_hip_load_fastx_files): wall %.3f s" % wall(lambda: e.load_fastx_files([wrapped]), a.reps))
        assert e.load_fastx_files([four]).n_reads == a.reads
        say("- one context, class 1, four-line: wall %.3f s" % wall(lambda: e.load_fastx_files([four]), a.reps))
    for n in (1, 2, 4):
        label = "a group of one rank" if n == 1 else "%d contexts sharing one GPU" % n
        with ca.SearchGroup([0] * n, local_copies=n > 1) as g:
            for r in range(n):
                g.rank_set_stage_timing(r, 1)
            assert g.load_fastx_files([four]).n_reads == a.reads and g.load_counters() == (1, 0, 0, 0)
            w0 = wall(lambda: g.load_fastx_files([four]), a.reps)
            g.set_fastq_class(1)
            assert g.load_fastx_files([four]).n_reads == a.reads and g.load_counters() == (1, 0, 0, 0)      # the one condition: one attempt
            w1 = wall(lambda: g.load_fastx_files([four]), a.reps)
            say("- %s, four-line: class 0 wall %.3f s, class 1 wall %.3f s (one attempt)" % (label, w0, w1))
            assert g.load_fastx_files([wrapped]).n_reads == a.reads
            cnt = g.load_counters()
            ms = [g.rank_last_cut_chain_ms(r) for r in range(n)]
            w2 = wall(lambda: g.load_fastx_files([wrapped]), a.reps)
            say("- %s, wrapped, class 1: wall %.3f s; attempts %d, files chained %d, margin doublings %d, look-ups %d; cut kernels %.3f ms summed over the ranks, %.3f ms the largest rank" % (
                label, w2, cnt[0], cnt[1], cnt[2], cnt[3], sum(ms), max(ms)))
    say("The contexts of a group here share one device, its copy engines and one host: the rows say what the route costs there, not how")
    say("it scales over real devices, which a one-GPU box cannot measure.")
    if OUT:
        OUT.close()


if __name__ == "__main__":
    main()
