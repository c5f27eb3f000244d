#!/usr/bin/env python3
"""What the wrapped FASTQ scan (fastx_wrapped.hip, crass_hip_set_fastq_class) costs.

Synthetic 150 bp reads (--reads N, default 2 M), median of --reps (5), wall seconds around the whole call (it returns when the
set is resident), in one process and in this order:
  (a) the general rule against the four-line scan on the same records, bytes already in HBM (crass_hip_attach_device_fastx):
      the four-line file with class 0, and the same file with ONE blank line appended with class 1 — the blank line is what the
      four-line scan declines, so the second figure is the four-line scan plus the wrapped scan, as a caller pays it
  (b) the same records wrapped at 60 columns (sequence and quality three lines each), host bytes, class 1
      (crass_hip_load_fastx_bytes) against the indexed reader (crass_index_fastx + crass_hip_load_reads) on the CPUs of the
      affinity mask
Output: stdout and --out (default profiles/wrapped_scan_mi355x.txt)."""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import crass_amd as ca

ca.load()
OUT = None


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def timed(fn, reps):
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
    return float(np.median(wall))


def make_files(n, L=150, W=60):
    """(four-line FASTQ, the same records wrapped at W columns) as uint8 arrays, built with numpy"""
    assert L % W == 30 and L // W == 2
    words = ca.synth_packed(ca.synth_spec(read_len=L), 0, n)
    asc = ca.unpack_ascii(words, (L + 15) // 16, L, n).reshape(n, L)
    digits = (np.arange(n, dtype=np.int64)[:, None] // 10 ** np.arange(7, -1, -1)) % 10 + ord("0")
    fq = np.empty((n, 1 + 8 + 1 + L + 1 + 2 + L + 1), np.uint8)
    fq[:, 0] = ord("@"); fq[:, 1:9] = digits; fq[:, 9] = 10; fq[:, 10:10 + L] = asc; fq[:, 10 + L] = 10
    fq[:, 11 + L] = ord("+"); fq[:, 12 + L] = 10; fq[:, 13 + L:13 + 2 * L] = ord("I"); fq[:, 13 + 2 * L] = 10
    lines = [asc[:, 0:60], asc[:, 60:120], asc[:, 120:150]]
    cols = [np.full((n, 1), ord("@"), np.uint8), digits.astype(np.uint8), np.full((n, 1), 10, np.uint8)]
    for ln in lines:
        cols += [ln, np.full((n, 1), 10, np.uint8)]
    cols += [np.full((n, 1), ord("+"), np.uint8), np.full((n, 1), 10, np.uint8)]
    for ln in lines:
        cols += [np.full(ln.shape, ord("I"), np.uint8), np.full((n, 1), 10, np.uint8)]
    return fq.reshape(-1), np.concatenate(cols, axis=1).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scratch", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wrapped_scan_mi355x.txt"))
    args = ap.parse_args()
    global OUT
    OUT = open(args.out, "w") if args.out else None
    n = args.reads
    say("%d CPUs in the affinity mask; device %s; %d reads of 150 bases" % (len(os.sched_getaffinity(0)), torch.cuda.get_device_name(0), n))
    four, wrapped = make_files(n)
    blank = np.concatenate([four, np.array([10], np.uint8)])
    with ca.SearchEngine(device=0) as e4, ca.SearchEngine(device=0) as e1:
        e1.set_fastq_class(1)
        d_four, d_blank = torch.from_numpy(four).to("cuda"), torch.from_numpy(blank).to("cuda")
        assert e4.attach_device_fastx(d_four).n_reads == n and e4.last_scan_classes() == (1, 0)
        assert e1.attach_device_fastx(d_blank).n_reads == n and e1.last_scan_classes() == (0, 1)
        a4 = timed(lambda: e4.attach_device_fastx(d_four), args.reps)
        a1 = timed(lambda: e1.attach_device_fastx(d_blank), args.reps)
        say("(a) four-line file, %.3f GB in HBM: four-line scan %.4f s; with a blank line, class 1 (four-line scan + wrapped scan) %.4f s; ratio %.2f"
            % (len(four) / 1e9, a4, a1, a1 / a4))
        del d_four, d_blank
        torch.cuda.empty_cache()
        with tempfile.TemporaryDirectory(dir=args.scratch) as scratch:
            path = os.path.join(scratch, "wrapped.fq")
            wrapped.tofile(path)

            def indexed():
                ix = ca.FastxIndex(path)
                e4.load_reads(ix)
                ix.close()
            indexed()
            assert e4.counters()["n_reads"] == n
            assert e1.load_fastx_bytes(wrapped).n_reads == n and e1.last_scan_classes() == (0, 1)
            b_ix = timed(indexed, args.reps)
            b_dev = timed(lambda: e1.load_fastx_bytes(wrapped), args.reps)
            say("(b) wrapped file, %.3f GB of host bytes: crass_hip_load_fastx_bytes, class 1 %.4f s (%.2f GB/s); crass_index_fastx + crass_hip_load_reads %.4f s; device / indexed %.2f"
                % (len(wrapped) / 1e9, b_dev, len(wrapped) / b_dev / 1e9, b_ix, b_dev / b_ix))


if __name__ == "__main__":
    main()
