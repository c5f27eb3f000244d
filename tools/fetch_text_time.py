#!/usr/bin/env python3
"""What it costs to get the text of the records of one step back out of the resident packed set (k_fetch_text, pack.hip).

Two inputs: synthetic 150 bp reads (10 M, or --reads N) and the same text cut into ragged reads of 100 .. 5 000 bases with
0.5 % 'N' reads.  The text goes in through crass_hip_attach_device_text, one step runs, then medians of five, in one process:
  (a) fetch_record_text(1) + fetch_record_text(2)      wall seconds of the two calls (getters, copies up, kernel, copy back,
                                                        the wait) and the two kernels alone (crass_hip_last_fetch_ms)
  (b) the same records from a HOST copy of the text    wall seconds: numpy gather of the reads' bytes + the host reverse
                                                        complement of the records that need it
  (c) hipMemcpyAsync device -> device of as many bytes HIP events on the context's stream: the streaming yardstick
(c) runs behind ~30 ms of unrelated device work on the same stream, so that the clocks are up (tools/idle_effect.py).
Output: stdout and profiles/fetch_text_mi355x.txt (--out)."""
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
COMP = np.arange(256, dtype=np.uint8) & 127
for _a, _b in zip(b"ACBDKRSWN", b"TGVHMYSWN"):
    for _x, _y in ((_a, _b), (_b, _a), (_a + 32, _b + 32), (_b + 32, _a + 32)):
        COMP[[_x, _x + 128]] = _y
COMP[[ord("U"), ord("U") + 128]] = ord("A")
COMP[[ord("u"), ord("u") + 128]] = ord("a")
COMP[[96, 224]] = 64


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def med(v):
    return float(np.median(v))


def host_records(buf, off, idx, low):
    """the records from a host copy of the text: chars and offsets like crass_text"""
    start, ln = off[idx].astype(np.int64), (off[idx + 1] - off[idx]).astype(np.int64)
    o = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(ln, out=o[1:])
    rc = np.repeat(low == 0, ln)
    # byte p of record k: forward start + p, reversed start + len - 1 - p
    k_of = np.repeat(np.arange(len(idx)), ln)
    p = np.arange(o[-1]) - o[k_of]
    src = np.where(rc, start[k_of] + ln[k_of] - 1 - p, start[k_of] + p)
    chars = buf[src]
    chars[rc] = COMP[chars[rc]]
    return chars, o


def measure(tag, buf, off, pad):
    n, nbytes = len(off) - 1, int(off[-1] - off[0])
    say("== %s: %d reads, %.3f GB of text" % (tag, n, nbytes / 1e9))
    eng = ca.SearchEngine(device=0)
    stream = torch.cuda.ExternalStream(eng.stream_handle())
    busy = torch.randn(4096, 4096, device="cuda", dtype=torch.float16)
    dev = torch.from_numpy(buf).to("cuda")
    eng.attach_device_text(dev, off, pad_uniform=pad)
    del dev
    torch.cuda.empty_cache()
    cand = eng.seed_scan()
    eng.merge()
    rec = eng.recruit()
    say("    one step: %d candidates, %d recruits (%.2f %% of the reads)" % (cand.n, rec.n, 100.0 * (cand.n + rec.n) / max(n, 1)))

    eng.set_stage_timing(1)
    for _ in range(2):                                   # warm-up: the pinned and device buffers of the result
        eng.fetch_record_text(1), eng.fetch_record_text(2)
    wall, kern, fetched = [], [], 0
    for _ in range(5):
        w0 = time.perf_counter()
        t1 = eng.fetch_record_text(1)
        k1, b1 = eng.last_fetch_ms(), int(t1.off[-1])
        t2 = eng.fetch_record_text(2)
        k2, b2 = eng.last_fetch_ms(), int(t2.off[-1])
        wall.append(time.perf_counter() - w0)
        kern.append((k1 + k2) / 1e3)
        fetched = b1 + b2
    a_wall, a_k = med(wall), med(kern)
    say("(a) fetch_record_text(1) + (2), %.4f GB            wall %.5f s   the two kernels %.6f s   %.1f GB/s written by the kernels"
        % (fetched / 1e9, a_wall, a_k, fetched / max(a_k, 1e-9) / 1e9))

    idx = np.concatenate([cand.read_idx, rec.read_idx]).astype(np.int64)
    low = np.concatenate([cand.low_lexi, rec.low_lexi])
    hw = []
    for _ in range(5):
        w0 = time.perf_counter()
        chars, o = host_records(buf, off, idx, low)
        hw.append(time.perf_counter() - w0)
    b_wall = med(hw)
    t1, t2 = eng.fetch_record_text(1), None
    same1 = np.array_equal(t1.chars, chars[:int(t1.off[-1])])
    t2 = eng.fetch_record_text(2)
    same2 = np.array_equal(t2.chars, chars[len(chars) - int(t2.off[-1]):])
    say("(b) the same records from a host copy (numpy)       wall %.5f s   [same bytes as (a): %s]" % (b_wall, same1 and same2))

    src = torch.empty(max(fetched, 1), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    ev = []
    for r in range(7):
        with torch.cuda.stream(stream):
            for _ in range(24):
                busy @ busy
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            dst.copy_(src, non_blocking=True)
            e1.record(stream)
        e1.synchronize()
        if r >= 2:
            ev.append(e0.elapsed_time(e1) / 1e3)
    c_ev = med(ev)
    say("(c) hipMemcpyAsync device -> device, %.4f GB       events %.6f s   %.1f GB/s read (+ as much written)" % (fetched / 1e9, c_ev, fetched / c_ev / 1e9))
    say("    (a, kernels) / (c) = %.2f   (a, wall) / (b, wall) = %.3f" % (a_k / c_ev, a_wall / b_wall))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--ragged-reads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fetch_text_mi355x.txt"))
    args = ap.parse_args()
    global OUT
    OUT = open(args.out, "w") if args.out else None
    say("%d CPUs in the affinity mask; device %s" % (len(os.sched_getaffinity(0)), torch.cuda.get_device_name(0)))
    n, L = args.reads, 150
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
