#!/usr/bin/env python3
"""What the comment kseq hands on costs on the device, against what a caller without it would do.

Two files of synthetic 150 bp reads as four-line FASTQ (--reads N in all, default 4 M; half in each file, the files of
tools/load_files_time.py with a comment on every third header line), loaded once with crass_hip_load_fastx_files.  Then, medians
of --reps (5), wall milliseconds and the HIP-event milliseconds of crass_hip_last_comments_ms (timing level 1):
  (a) crass_hip_fastx_comments_build_device on the arena      k_cm_bits / k_cm_tiles / k_cm_top, the record positions up
  (b) crass_hip_fetch_comments_device of 1 % of the records   k_cm_source / k_cm_measure / k_span_copy, drawn without order
  (c) the arena copied back to the host + crass_fastx_comments_of for the same records       what (a) + (b) replace
and whether (b) and (c) agree byte for byte.  Output: stdout and profiles/comments_time_mi355x.txt (--out)."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import crass_amd as ca

ca.load()
OUT = None


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def fastq_bytes(first, n, L):
    """n (a multiple of 3) synthetic reads from read `first` on as a four-line FASTQ, built with numpy: '@' + an 8-digit name, on
    every third record ' c' + the 8 digits again, the read, '+', 'I' * L"""
    spec = ca.synth_spec(read_len=L, crispr_per_million=10000)
    asc = ca.unpack_ascii(ca.synth_packed(spec, first, n), (L + 15) // 16, L, n).reshape(n, L)
    idx = np.arange(first, first + n, dtype=np.int64)

    def records(rows, comment):
        h = 1 + 8 + (10 if comment else 0)
        rec = np.empty((len(rows), h + 1 + L + 3 + L + 1), np.uint8)
        rec[:, 0] = ord("@")
        for d in range(8):
            rec[:, 8 - d] = ord("0") + (idx[rows] // 10 ** d) % 10
        if comment:
            rec[:, 9:11] = np.frombuffer(b" c", np.uint8)
            rec[:, 11:19] = rec[:, 1:9]
        rec[:, h] = 10
        rec[:, h + 1:h + 1 + L] = asc[rows]
        rec[:, h + 1 + L:h + 4 + L] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, h + 4 + L:h + 4 + 2 * L] = ord("I")
        rec[:, h + 4 + 2 * L] = 10
        return rec
    rows = np.arange(n)
    return np.concatenate([records(rows[0::3], True), records(rows[1::3], False), records(rows[2::3], False)], axis=1).tobytes()


def timed(fn, reps, ms):
    wall, dev = [], []
    for _ in range(reps):
        w0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - w0) * 1e3)
        dev.append(ms())
    return float(np.median(wall)), float(np.median(dev))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "comments_time_mi355x.txt"))
    a = ap.parse_args()
    OUT = open(a.out, "w")
    half = a.reads // 2 // 3 * 3
    bufs = [np.frombuffer(fastq_bytes(0, half, a.len), np.uint8), np.frombuffer(fastq_bytes(half, half, a.len), np.uint8)]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    with ca.SearchEngine() as e:
        e.set_stage_timing(1)
        lay = e.load_fastx_files(bufs)
        addr, nb = e.resident_fastx()
        n = lay.n_reads
        say("two files, %d + %d reads of %d bp, a comment on every third record; arena %.3f GB" % (half, half, a.len, nb / 1e9))
        idx = np.random.default_rng(26).choice(n, n // 100, replace=False).astype(np.uint64)
        e.comments_build()
        e.fetch_comments(idx)                                 # (first calls: allocations, code objects)
        wa, da = timed(e.comments_build, a.reps, lambda: e.last_comments_ms()[0])
        own, recs = e.comments_counters()
        say("(a) build on the arena            wall %8.3f ms   kernels %8.3f ms   (%d of %d records have a comment of their own; kept: %d bytes)" % (
            wa, da, own, recs, (n + 63) // 64 * 8 + (n + 4095) // 4096 * 8 + 8 * len(lay.file_read_base)))
        got = [None]

        def fetch():
            got[0] = e.fetch_comments(idx)
        wb, db = timed(fetch, a.reps, lambda: e.last_comments_ms()[1])
        say("(b) fetch of %7d records      wall %8.3f ms   kernels and the copies between them %8.3f ms   (%d bytes)" % (len(idx), wb, db, int(got[0][1][-1])))
        host = np.empty(nb, np.uint8)
        ref = [None]

        def back():
            assert hip.hipMemcpy(host.ctypes.data, addr, nb, 2) == 0
            ref[0] = ca.comments_of(host, lay.rec_pos, idx, lay.file_read_base)
        wc, _ = timed(back, a.reps, lambda: 0.0)
        w0 = time.perf_counter()
        assert hip.hipMemcpy(host.ctypes.data, addr, nb, 2) == 0
        wcopy = (time.perf_counter() - w0) * 1e3
        say("(c) arena to the host + crass_fastx_comments_of   wall %8.3f ms   (the copy alone, once: %.3f ms)" % (wc, wcopy))
        same = all(np.array_equal(x, y) for x, y in zip(got[0], ref[0]))
        say("(b) and (c) agree byte for byte: %s; (c) / ((a) + (b)) = %.1f" % (same, wc / (wa + wb) if wa + wb else 0.0))
    OUT.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
