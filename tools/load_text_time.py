#!/usr/bin/env python3
"""What it costs to get sequence TEXT resident as packed reads: the host route against the device packer (pack.hip).

Two inputs: synthetic 150 bp reads (50 M; 10 M when the host is short of memory, or --reads N) and ragged reads of
100 .. 5 000 bases with 0.5 % 'N' reads.  Median of five, in one process and in this order:
  (a) crass_pack_reads + crass_hip_load_reads           wall and CPU seconds (today's only way to the same resident bytes)
  (b) crass_hip_load_text from pageable memory          wall and CPU seconds
  (c) crass_hip_load_text from pinned memory            wall and CPU seconds
  (d) crass_hip_attach_device_text, the whole call      HIP events on the context's stream, and wall; and its pack kernel
                                                        alone (crass_hip_last_pack_ms: events around the kernel, timing level 1)
  (e) hipMemcpyAsync device -> device of the text bytes HIP events on the context's stream: the streaming yardstick
(d) and (e) run after warm-up behind ~30 ms of unrelated device work on the same stream, so that the clocks are up when
the timed work starts (tools/idle_effect.py).  Output: stdout and profiles/load_text_mi355x.txt (--out)."""
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


def say(text, flush=True):
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


def timed_host(fn, reps=5):
    wall, cpu = [], []
    for _ in range(reps):
        w0, c0 = time.perf_counter(), time.process_time()
        fn()
        wall.append(time.perf_counter() - w0)
        cpu.append(time.process_time() - c0)
    return med(wall), med(cpu)


def measure(tag, buf, off, pad):
    n, nbytes = len(off) - 1, int(off[-1] - off[0])
    say("== %s: %d reads, %.3f GB of text" % (tag, n, nbytes / 1e9), flush=True)
    eng = ca.SearchEngine(device=0)
    stream = torch.cuda.ExternalStream(eng.stream_handle())
    busy = torch.randn(4096, 4096, device="cuda", dtype=torch.float16)

    def route_a():
        pk = ca.PackedReads((buf, off), pad_uniform=pad)
        eng.load_reads(pk)
        pk.close()
    route_a()                                            # warm-up: allocations, code objects, page faults of the result buffers
    a_wall, a_cpu = timed_host(route_a)
    words = eng.counters()["bytes_reads_device"]
    say("(a) crass_pack_reads + crass_hip_load_reads      wall %.4f s   cpu %.4f s   (%.3f GB packed)" % (a_wall, a_cpu, words / 1e9), flush=True)

    eng.load_text((buf, off), pad_uniform=pad)
    b_wall, b_cpu = timed_host(lambda: eng.load_text((buf, off), pad_uniform=pad))
    say("(b) crass_hip_load_text, pageable text            wall %.4f s   cpu %.4f s   %.2f GB/s of text" % (b_wall, b_cpu, nbytes / b_wall / 1e9), flush=True)

    pinned = torch.from_numpy(buf).pin_memory()
    pbuf = pinned.numpy()
    eng.load_text((pbuf, off), pad_uniform=pad)
    c_wall, c_cpu = timed_host(lambda: eng.load_text((pbuf, off), pad_uniform=pad))
    say("(c) crass_hip_load_text, pinned text              wall %.4f s   cpu %.4f s   %.2f GB/s of text" % (c_wall, c_cpu, nbytes / c_wall / 1e9), flush=True)

    dev = pinned.to("cuda", non_blocking=False)
    del pinned, pbuf
    dst = torch.empty_like(dev)

    def front():                                         # ~30 ms of unrelated work on the context's stream
        with torch.cuda.stream(stream):
            for _ in range(24):
                busy @ busy

    def timed_dev(fn, reps=5):
        ev_ms, wall = [], []
        for _ in range(reps):
            front()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            w0 = time.perf_counter()
            fn()
            e1.record(stream)
            e1.synchronize()
            wall.append(time.perf_counter() - w0)
            ev_ms.append(e0.elapsed_time(e1))
        return med(ev_ms) / 1e3, med(wall)

    for _ in range(2):
        eng.attach_device_text(dev, off, pad_uniform=pad)
    eng.set_stage_timing(1)
    d_kern = []

    def attach():
        eng.attach_device_text(dev, off, pad_uniform=pad)
        d_kern.append(eng.last_pack_ms() / 1e3)
    d_ev, d_wall = timed_dev(attach)
    d_k = med(d_kern)
    eng.set_stage_timing(0)
    say("(d) crass_hip_attach_device_text, whole call      events %.5f s   wall (behind the queued work) %.5f s   %.1f GB/s of text by the events"
        % (d_ev, d_wall, nbytes / d_ev / 1e9), flush=True)
    say("(d) ... its pack kernel alone                     events %.5f s   %.1f GB/s of text read, %.1f GB/s read + written"
        % (d_k, nbytes / d_k / 1e9, (nbytes + words) / d_k / 1e9), flush=True)

    def d2d():
        with torch.cuda.stream(stream):
            dst.copy_(dev, non_blocking=True)
    for _ in range(2):
        d2d()
    e_ev, _ = timed_dev(d2d)
    say("(e) hipMemcpyAsync device -> device, %.3f GB     events %.5f s   %.1f GB/s read (+ as much written)" % (nbytes / 1e9, e_ev, nbytes / e_ev / 1e9), flush=True)
    say("    (d) / (a) wall = %.4f   [(d) < (a): %s]   (d) / (e) = %.2f   (d, kernel only) / (e) = %.2f   (b) / (a) wall = %.2f, cpu = %.2f   (c) / (a) wall = %.2f, cpu = %.2f"
        % (d_ev / a_wall, d_ev < a_wall, d_ev / e_ev, d_k / e_ev, b_wall / a_wall, b_cpu / max(a_cpu, 1e-9), c_wall / a_wall, c_cpu / max(a_cpu, 1e-9)), flush=True)
    cnt = eng.counters()
    say("    resident: %d reads, %d exception reads, %.3f GB packed" % (cnt["n_reads"], cnt["n_exceptions"], cnt["bytes_reads_device"] / 1e9), flush=True)
    eng.close()
    del dev, dst
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="150 bp reads (default: 50 M, 10 M on a host with less than 96 GB available)")
    ap.add_argument("--ragged-reads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "load_text_mi355x.txt"))
    args = ap.parse_args()
    global OUT
    OUT = open(args.out, "w") if args.out else None
    avail = mem_available_gb()
    n = args.reads or (50_000_000 if avail >= 96 else 10_000_000)
    say("host memory available %.0f GB, %d CPUs in the affinity mask; device %s" % (avail, len(os.sched_getaffinity(0)), torch.cuda.get_device_name(0)), flush=True)
    L = 150
    words = ca.synth_packed(ca.synth_spec(read_len=L), 0, n)
    buf = ca.unpack_ascii(words, (L + 15) // 16, L, n)
    del words
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    measure("synthetic %d x %d bp" % (n, L), buf, off, 2)
    # ragged: the same text cut at other places (100 .. 5 000 bases), one 'N' in 0.5 % of the reads
    rng = np.random.default_rng(9)
    m = args.ragged_reads
    lens = rng.integers(100, 5001, size=m).astype(np.uint64)
    roff = np.zeros(m + 1, dtype=np.uint64)
    roff[1:] = np.cumsum(lens)
    keep = int(np.searchsorted(roff, len(buf), side="right")) - 1
    roff = roff[:keep + 1].copy()
    rbuf = buf[:int(roff[-1])].copy()
    del buf
    nn = rng.choice(keep, size=max(1, keep // 200), replace=False)
    rbuf[(roff[nn] + (rng.integers(0, 100, size=len(nn))).astype(np.uint64)).astype(np.int64)] = ord("N")
    measure("ragged %d reads of 100 .. 5 000 bases, 0.5 %% with an N" % keep, rbuf, roff, 2)


if __name__ == "__main__":
    main()
