#!/usr/bin/env python3
"""What it costs to turn names that come from elsewhere into record indices of a FASTQ whose bytes live on the device: the name
table kept on the device (crass_hip_fastx_names_build_device, crass_hip_fastx_names_find; fastx_hid.hip) against the host
function on host bytes, and the copy back a caller pays without it.

Synthetic FASTQ built with numpy, fixed-width records ('@' + 'r' + nine digits + ' ' + mate + '\\n' + 50 bases + '\\n+\\n' + 50
quality bytes + '\\n'), so the record positions are known without a scan; --reads in millions (default 2,8).  One name in a
hundred is queried (--frac), half of the queries with their last digit replaced by a letter, so that they are absent.  Per input:
  (a) crass_fastx_find_names on the host bytes                     wall seconds (one thread: the table and the lookups)
  (b) names_build on a device tensor                               HIP events of the insert launches; wall of the call
  (c) names_find on that table                                     HIP events of the two find kernels; wall of the call (upload of
                                                                    the queries and copy back of the answers included)
  (d) the file's bytes device -> host                              wall into pageable memory, events into pinned memory
(c)'s answers are compared with (a)'s.  Output: stdout and profiles/find_names_mi355x.txt (--out)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import crass_amd as ca

ca.load()
OUT = None
L = 50
W = 1 + 1 + 9 + 1 + 1 + 1 + L + 3 + L + 1


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def med(v):
    return float(np.median(v))


def make_file(n):
    rng = np.random.default_rng(5)
    rec = np.empty((n, W), np.uint8)
    ids = np.arange(n, dtype=np.int64)
    rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
    for k in range(9):
        rec[:, 2 + k] = (ids // 10 ** (8 - k)) % 10 + ord("0")
    rec[:, 11] = ord(" "); rec[:, 12] = ord("1"); rec[:, 13] = 10
    rec[:, 14:14 + L] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]
    rec[:, 14 + L:17 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 17 + L:17 + 2 * L] = ord("I")
    rec[:, 17 + 2 * L] = 10
    return rec.reshape(-1), np.arange(n + 1, dtype=np.uint64) * W


def make_queries(data, n, frac):
    rng = np.random.default_rng(7)
    m = max(1, int(n * frac))
    pick = rng.choice(n, m, replace=False)
    names = data.reshape(n, W)[pick, 1:11].copy()          # 'r' + nine digits
    names[::2, 9] = ord("x")                               # every other one: absent
    return names.reshape(-1), np.arange(m + 1, dtype=np.uint64) * 10, pick


def measure(eng, n, frac, reps):
    data, rec_pos = make_file(n)
    nbytes = len(data)
    chars, off, pick = make_queries(data, n, frac)
    m = len(off) - 1
    slots = 2
    while slots < 2 * n:
        slots <<= 1
    say("== %d reads, %d queries: %.3f GB of file bytes, kept on the device: table %.3f GB + record positions %.3f GB"
        % (n, m, nbytes / 1e9, slots * 8 / 1e9, n * 8 / 1e9))
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        want = ca.find_names(data, rec_pos, (chars, off))
        wall.append(time.perf_counter() - t0)
    a_wall = med(wall)
    expect = np.where(np.arange(m) % 2 == 0, np.uint64(2 ** 64 - 1), pick.astype(np.uint64))
    assert np.array_equal(want, expect)
    say("(a) crass_fastx_find_names, host bytes          wall %.4f s" % a_wall)

    dev = torch.from_numpy(data).to("cuda")
    torch.cuda.synchronize()
    eng.names_build(dev, rec_pos)                          # (warm: first-use costs of the kernels)
    assert np.array_equal(eng.names_find((chars, off)), want)
    eng.set_stage_timing(1)
    b_ev, b_wall, c_ev, c_wall = [], [], [], []
    for _ in range(max(reps, 3)):
        t0 = time.perf_counter()
        eng.names_build(dev, rec_pos)
        b_wall.append(time.perf_counter() - t0)
        b_ev.append(eng.last_names_ms()[0])
        t0 = time.perf_counter()
        got = eng.names_find((chars, off))
        c_wall.append(time.perf_counter() - t0)
        c_ev.append(eng.last_names_ms()[1])
        assert np.array_equal(got, want)
    eng.set_stage_timing(0)
    eng.names_drop()
    say("(b) names_build, device bytes                   events %.3f ms (%.1f M reads/s)   wall %.4f s" % (med(b_ev), n / med(b_ev) / 1e3, med(b_wall)))
    say("(c) names_find, %9d queries               events %.3f ms (%.1f M queries/s)   wall %.4f s" % (m, med(c_ev), m / med(c_ev) / 1e3, med(c_wall)))

    wall = []
    for _ in range(max(reps, 3)):
        t0 = time.perf_counter()
        back = dev.cpu()
        wall.append(time.perf_counter() - t0)
        del back
    pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    evs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pinned.copy_(dev, non_blocking=True)
        e1.record()
        e1.synchronize()
        evs.append(e0.elapsed_time(e1))
    d_wall, d_ms = med(wall), med(evs[1:])
    say("(d) the file's bytes device -> host             wall %.4f s pageable; events %.3f ms pinned (%.1f GB/s)" % (d_wall, d_ms, nbytes / d_ms / 1e6))
    say("    without the table (d) + (a) = %.4f s; with it (b) + (c) = %.4f s wall" % (d_wall + a_wall, med(b_wall) + med(c_wall)))
    del dev, pinned
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", default="2,8", help="millions of reads, comma-separated")
    ap.add_argument("--frac", type=float, default=0.01, help="share of the names that is queried")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "find_names_mi355x.txt"))
    args = ap.parse_args()
    global OUT
    OUT = open(args.out, "w") if args.out else None
    say("device %s; records of %d bytes; medians of %d runs" % (torch.cuda.get_device_name(0), W, max(args.reps, 3)))
    with ca.SearchEngine(device=0) as eng:
        for mreads in [float(x) for x in args.reads.split(",") if x]:
            measure(eng, int(mreads * 1e6), args.frac, args.reps)


if __name__ == "__main__":
    main()
