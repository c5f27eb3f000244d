#!/usr/bin/env python3
"""What it costs to get the BYTES of a FASTA / FASTQ file resident as packed reads: the two host readers against the device
record scan (fastx_scan.hip).

Two inputs held in memory (and written once to a scratch file for the readers that take a path): synthetic 150 bp reads as a
one-line FASTA and as a four-line FASTQ (--reads N, default 10 M; 2 M on a host with less than 32 GB available).  Median of
--reps (3), in one process and in this order, wall and CPU seconds each:
  (a) crass_index_fastx + crass_hip_load_reads             the indexed reader (parses and packs on the host, many threads)
  (b) crass_read_fastx + crass_hip_load_text               the whole-file reader, packed on the device
  (c) crass_hip_load_fastx_bytes                           the bytes go up as they are; scan and pack on the device
  (d) crass_hip_attach_device_fastx                        the same for bytes that are already in HBM
and crass_hip_last_scan_ms / crass_hip_last_pack_ms of (d) (HIP events, timing level 1) against
  (e) hipMemcpyAsync device -> device of the file's bytes   the streaming yardstick: a kernel that reads and writes the bytes once
Output: stdout and profiles/load_fastx_mi355x.txt (--out)."""
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


def mem_available_gb():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) / 1e6
    return 0.0


def med(v):
    return float(np.median(v))


def timed_host(fn, reps):
    wall, cpu = [], []
    for _ in range(reps):
        w0, c0 = time.perf_counter(), time.process_time()
        fn()
        wall.append(time.perf_counter() - w0)
        cpu.append(time.process_time() - c0)
    return med(wall), med(cpu)


def make_files(n, L):
    """(fasta bytes, fastq bytes) as uint8 arrays, built with numpy: '>' / '@' + an 8-digit name, the read, and for FASTQ '+' and
    a quality line"""
    words = ca.synth_packed(ca.synth_spec(read_len=L), 0, n)
    asc = ca.unpack_ascii(words, (L + 15) // 16, L, n).reshape(n, L)
    del words
    digits = (np.arange(n, dtype=np.int64)[:, None] // 10 ** np.arange(7, -1, -1)) % 10 + ord("0")
    fa = np.empty((n, 1 + 8 + 1 + L + 1), np.uint8)
    fa[:, 0] = ord(">"); fa[:, 1:9] = digits; fa[:, 9] = 10; fa[:, 10:10 + L] = asc; fa[:, 10 + L] = 10
    fq = np.empty((n, 1 + 8 + 1 + L + 1 + 2 + L + 1), np.uint8)
    fq[:, 0] = ord("@"); fq[:, 1:9] = digits; fq[:, 9] = 10; fq[:, 10:10 + L] = asc; fq[:, 10 + L] = 10
    fq[:, 11 + L] = ord("+"); fq[:, 12 + L] = 10; fq[:, 13 + L:13 + 2 * L] = ord("I"); fq[:, 13 + 2 * L] = 10
    return fa.reshape(-1), fq.reshape(-1)


def measure(tag, data, scratch, reps):
    nbytes = len(data)
    path = os.path.join(scratch, tag + ".fx")
    data.tofile(path)
    say("== %s: %.3f GB of file bytes" % (tag, nbytes / 1e9))
    eng = ca.SearchEngine(device=0)
    stream = torch.cuda.ExternalStream(eng.stream_handle())

    def route_a():
        ix = ca.FastxIndex(path)
        eng.load_reads(ix)
        ix.close()
    route_a()
    a_wall, a_cpu = timed_host(route_a, reps)
    cnt = eng.counters()
    n_reads, words = cnt["n_reads"], cnt["bytes_reads_device"]
    say("(a) crass_index_fastx + crass_hip_load_reads          wall %.4f s   cpu %.4f s   (%d reads, %.3f GB packed)" % (a_wall, a_cpu, n_reads, words / 1e9))

    lib = eng.lib

    def route_b():
        import ctypes as C
        f = ca._abi.Fastx()
        ca.engine._chk(lib.crass_read_fastx(path.encode(), C.byref(f)), "crass_read_fastx")
        ca.engine._chk(lib.crass_hip_load_text(eng.h, f.seq, f.seq_off, f.n_reads, 2, None, 0), "crass_hip_load_text")
        lib.crass_free_fastx(C.byref(f))
    route_b()
    b_wall, b_cpu = timed_host(route_b, reps)
    say("(b) crass_read_fastx + crass_hip_load_text            wall %.4f s   cpu %.4f s" % (b_wall, b_cpu))

    lay = eng.load_fastx_bytes(data)
    assert lay.n_reads == n_reads and eng.counters()["bytes_reads_device"] == words
    c_wall, c_cpu = timed_host(lambda: eng.load_fastx_bytes(data), reps)
    say("(c) crass_hip_load_fastx_bytes, pageable bytes        wall %.4f s   cpu %.4f s   %.2f GB/s of file bytes" % (c_wall, c_cpu, nbytes / c_wall / 1e9))

    dev = torch.from_numpy(data).to("cuda")
    eng.attach_device_fastx(dev)
    eng.set_stage_timing(1)
    scan_ms, pack_ms = [], []

    def route_d():
        eng.attach_device_fastx(dev)
        scan_ms.append(eng.last_scan_ms())
        pack_ms.append(eng.last_pack_ms())
    d_wall, d_cpu = timed_host(route_d, max(reps, 5))
    eng.set_stage_timing(0)
    s_ms, p_ms = med(scan_ms), med(pack_ms)
    say("(d) crass_hip_attach_device_fastx, whole call         wall %.4f s   cpu %.4f s   %.1f GB/s of file bytes" % (d_wall, d_cpu, nbytes / d_wall / 1e9))
    say("(d) ... crass_hip_last_scan_ms %.3f (%.1f GB/s of file bytes, two passes over them)   crass_hip_last_pack_ms %.3f" % (s_ms, nbytes / s_ms / 1e6, p_ms))

    dst = torch.empty_like(dev)
    ev = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            dst.copy_(dev, non_blocking=True)
            e1.record(stream)
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    e_ms = med(ev[2:])
    say("(e) hipMemcpyAsync device -> device, %.3f GB         events %.3f ms   %.1f GB/s read (+ as much written)" % (nbytes / 1e9, e_ms, nbytes / e_ms / 1e6))
    say("    scan / copy = %.2f   (scan + pack) / copy = %.2f   (c) / (a) wall = %.2f, cpu = %.2f   (c) / (b) wall = %.2f, cpu = %.2f   [(c) < (a) on wall: %s]"
        % (s_ms / e_ms, (s_ms + p_ms) / e_ms, c_wall / a_wall, c_cpu / max(a_cpu, 1e-9), c_wall / b_wall, c_cpu / max(b_cpu, 1e-9), c_wall < a_wall))
    eng.close()
    os.unlink(path)
    del dev, dst
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scratch", default=None, help="directory for the scratch copies of the two files (default: a temporary one)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "load_fastx_mi355x.txt"))
    args = ap.parse_args()
    global OUT
    OUT = open(args.out, "w") if args.out else None
    avail = mem_available_gb()
    n = args.reads or (10_000_000 if avail >= 32 else 2_000_000)
    say("host memory available %.0f GB, %d CPUs in the affinity mask; device %s; %d reads of 150 bases" % (avail, len(os.sched_getaffinity(0)), torch.cuda.get_device_name(0), n))
    fa, fq = make_files(n, 150)
    with tempfile.TemporaryDirectory(dir=args.scratch) as scratch:
        measure("fasta", fa, scratch, args.reps)
        del fa
        measure("fastq", fq, scratch, args.reps)


if __name__ == "__main__":
    main()
