#!/usr/bin/env python3
"""What header ids cost a caller whose FASTA bytes live on the device: the host function on host bytes against the device call
(fastx_hid.hip), and the copy back such a caller pays today to feed the host function.

Synthetic FASTA built with numpy, fixed-width records ('>' + 'r' + nine digits + ' ' + mate + '\\n' + 50 bases + '\\n'), so the
record positions are known without a scan; --reads in millions (default 1,10,50; sizes that do not fit half of the available
host memory are skipped and said so), names unique (read i is r<i>) and paired (reads 2 k and 2 k + 1 are r<k>).  Per input:
  (a) crass_fastx_header_ids on the host bytes                     wall seconds (one thread)
  (b) crass_hip_fastx_header_ids_device on a device tensor         HIP events on the context's stream: all kernels, the insert
                                                                    launches, the lookup launch; wall of the whole call with the
                                                                    ids copied back, and without (header_id_out NULL)
  (c) the file's bytes device -> host                              wall into pageable memory, events into pinned memory
and the bytes of the name table.  (b)'s ids are compared with (a)'s.  Output: stdout and profiles/header_ids_mi355x.txt (--out)."""
import argparse
import ctypes as C
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
W = 1 + 1 + 9 + 1 + 1 + 1 + L + 1


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def mem_available_gb():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) / 1e6
    return 0.0


def med(v):
    return float(np.median(v))


def make_file(n, paired):
    rng = np.random.default_rng(5)
    rec = np.empty((n, W), np.uint8)
    ids = np.arange(n, dtype=np.int64)
    name = ids // 2 if paired else ids
    rec[:, 0] = ord(">"); rec[:, 1] = ord("r")
    for k in range(9):
        rec[:, 2 + k] = (name // 10 ** (8 - k)) % 10 + ord("0")
    rec[:, 11] = ord(" "); rec[:, 12] = (ids % 2 if paired else 0) + ord("1"); rec[:, 13] = 10
    rec[:, 14:14 + L] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)]
    rec[:, 14 + L] = 10
    return rec.reshape(-1), np.arange(n + 1, dtype=np.uint64) * W


def measure(eng, n, paired, reps):
    data, rec_pos = make_file(n, paired)
    nbytes = len(data)
    slots = 2
    while slots < 2 * n:
        slots <<= 1
    say("== %d reads, %s names: %.3f GB of file bytes, name table %.3f GB (%d slots of 8 bytes = %.1f bytes per read)"
        % (n, "paired" if paired else "unique", nbytes / 1e9, slots * 8 / 1e9, slots, slots * 8 / n))
    host_reps = reps if n <= 10_000_000 else 1
    wall = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = ca.fastx_header_ids(data, rec_pos)
        wall.append(time.perf_counter() - t0)
    a_wall = med(wall)
    say("(a) crass_fastx_header_ids, host bytes                  wall %.4f s (%d run%s)   %.1f M reads/s" % (a_wall, host_reps, "" if host_reps == 1 else "s", n / a_wall / 1e6))

    dev = torch.from_numpy(data).to("cuda")
    torch.cuda.synchronize()
    ids, n_rep = eng.device_header_ids(dev, rec_pos, install=False)      # (warm: first-use costs of the kernels)
    assert np.array_equal(ids, want) and n_rep == (n // 2 if paired else 0)
    eng.set_stage_timing(1)
    ev, wall, wall_noids = [], [], []
    for _ in range(max(reps, 3)):
        t0 = time.perf_counter()
        eng.device_header_ids(dev, rec_pos, install=False)
        wall.append(time.perf_counter() - t0)
        ev.append(eng.last_header_ids_ms())
        rep = C.c_uint64()
        t0 = time.perf_counter()
        st = eng.lib.crass_hip_fastx_header_ids_device(eng.h, int(dev.data_ptr()), nbytes, rec_pos.ctypes.data, n, None, 0, C.byref(rep))
        wall_noids.append(time.perf_counter() - t0)
        assert st == 0 and rep.value == n_rep
    eng.set_stage_timing(0)
    whole, ins, look = (med([e[k] for e in ev]) for k in range(3))
    say("(b) crass_hip_fastx_header_ids_device, device bytes     events %.3f ms = insert %.3f + lookup %.3f   %.1f M reads/s   %.1f GB/s of file bytes"
        % (whole, ins, look, n / whole / 1e3, nbytes / whole / 1e6))
    say("(b) ... the whole call                                  wall %.4f s with the ids copied back, %.4f s without" % (med(wall), med(wall_noids)))

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
    c_wall, c_ms = med(wall), med(evs[1:])
    say("(c) the file's bytes device -> host                     wall %.4f s pageable; events %.3f ms pinned (%.1f GB/s)" % (c_wall, c_ms, nbytes / c_ms / 1e6))
    say("    today (c) + (a) = %.4f s; the device call %.4f s; (a) / (b) events = %.1f   [(b) faster than (a): %s]"
        % (c_wall + a_wall, med(wall_noids), a_wall * 1e3 / whole, whole < a_wall * 1e3))
    del dev, pinned
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", default="1,10,50", help="millions of reads, comma-separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "header_ids_mi355x.txt"))
    args = ap.parse_args()
    global OUT
    OUT = open(args.out, "w") if args.out else None
    say("host memory available %.0f GB, %d CPUs in the affinity mask; device %s; records of %d bytes" % (mem_available_gb(), len(os.sched_getaffinity(0)), torch.cuda.get_device_name(0), W))
    with ca.SearchEngine(device=0) as eng:
        for m in [float(x) for x in args.reads.split(",") if x]:
            n = int(m * 1e6)
            need = 3.5 * n * W / 1e9                    # the file, its pinned copy, a pageable copy back, the ids
            if need > 0.5 * mem_available_gb():
                say("== %d reads skipped: about %.0f GB of host memory needed, %.0f available" % (n, need, mem_available_gb()))
                continue
            for paired in (False, True):
                measure(eng, n, paired, args.reps)


if __name__ == "__main__":
    main()
