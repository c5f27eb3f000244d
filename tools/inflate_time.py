#!/usr/bin/env python3
"""What it costs to get a BGZF-compressed FASTQ resident as packed reads: the device inflate (inflate.hip) in front of the device
record scan, against the host's side-by-side inflate, and against the upload of the already-inflated text.

One input held in memory (and written once to a scratch file for the reader that takes a path): a synthetic four-line FASTQ of
150 bp reads, --text-gb (default 1.0) of text, as BGZF members of 65 280 bytes at zlib level 6.  Median of --reps (3), one process:
  (a') the inflate kernel with the member's window in LDS (CRASS_INFLATE_WINDOW=lds) instead of in HBM, the default: event time
  (a) SearchEngine.load_fastx_bgzf            wall seconds; and with timing level 1 its parts: compressed bytes up (a timed copy of
                                              the same bytes), crass_hip_last_inflate_ms, crass_hip_last_scan_ms, crass_hip_last_pack_ms
  (b) crass_index_fastx on the same file      the host's side-by-side inflate + parse + pack (CRASS_TIMING=1 prints its stage times
                                              to stderr), then crass_hip_load_reads
  (c) SearchEngine.load_fastx_bytes           on the already-inflated text: what the H2D copy of 6-8 x the bytes costs
Output: stdout and profiles/inflate_mi355x.txt (--out): seconds, and bytes of TEXT per second for the inflate kernel."""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import crass_amd as ca
from tests import bgzf_sets

ca.load()


def med(v):
    return float(np.median(v))


def make_text(n_bytes, seed=14):
    rng = np.random.default_rng(seed)
    L = 150
    n = max(1, n_bytes // (2 * L + 20))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, L))]
    qual = np.frombuffer(b"FFFFF:,#", np.uint8)[rng.integers(0, 8, (n, L))]
    rec = np.full((n, 2 * L + 20), 10, np.uint8)         # '@' + 14 name bytes + '\n' + seq + '\n+\n' + qual + '\n'
    rec[:, 0] = ord("@")
    rec[:, 1:15] = np.frombuffer(b"".join(b"r%013d" % i for i in range(n)), np.uint8).reshape(n, 14)
    rec[:, 16:16 + L] = seq
    rec[:, 17 + L] = ord("+")
    rec[:, 19 + L:19 + 2 * L] = qual
    return rec.reshape(-1).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-gb", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "inflate_mi355x.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def say(t):
        print(t, flush=True)
        out.write(t + "\n")
        out.flush()

    text = make_text(int(a.text_gb * 1e9))
    t0 = time.perf_counter()
    data = bgzf_sets.bgzf(text, block=65280, level=6)
    say("text %.3f GB, BGZF %.3f GB (%.2f x), %d members, compressed in %.1f s" % (len(text) / 1e9, len(data) / 1e9, len(text) / len(data),
                                                                                  ca.bgzf_index(data).n_members, time.perf_counter() - t0))
    arr, tarr = np.frombuffer(data, np.uint8).copy(), np.frombuffer(text, np.uint8)
    for window in ("lds",):                               # the other placement of the member's window: the inflate kernel's time only
        os.environ["CRASS_INFLATE_WINDOW"] = window
        try:
            e = ca.SearchEngine()
        finally:
            os.environ.pop("CRASS_INFLATE_WINDOW", None)
        with e:
            e.set_stage_timing(1)
            e.load_fastx_bgzf(arr)
            ms = []
            for _ in range(a.reps):
                e.load_fastx_bgzf(arr)
                ms.append(e.last_inflate_ms() / 1e3)
            say("(a') window in %s: inflate %.3f s, %.2f GB of text per second" % (window.upper(), med(ms), len(text) / 1e9 / med(ms)))
    with ca.SearchEngine() as e:
        e.set_stage_timing(1)
        e.load_fastx_bgzf(arr)                            # warm: allocations, code objects
        wall, infl, scan, pack, up = [], [], [], [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lay = e.load_fastx_bgzf(arr)
            wall.append(time.perf_counter() - t0)
            infl.append(e.last_inflate_ms() / 1e3); scan.append(e.last_scan_ms() / 1e3); pack.append(e.last_pack_ms() / 1e3)
            t0 = time.perf_counter()
            torch.from_numpy(arr).to("cuda")
            torch.cuda.synchronize()
            up.append(time.perf_counter() - t0)
        say("(a) load_fastx_bgzf: wall %.3f s = compressed bytes up %.3f + inflate %.3f + scan %.3f + pack %.3f (+ host index, waits); %d reads" %
            (med(wall), med(up), med(infl), med(scan), med(pack), lay.n_reads))
        say("    inflate kernel: %.2f GB of text per second" % (len(text) / 1e9 / med(infl)))
        w = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            e.load_fastx_bytes(tarr)
            w.append(time.perf_counter() - t0)
        say("(c) load_fastx_bytes on the inflated text: wall %.3f s (scan %.3f, pack %.3f)" % (med(w), e.last_scan_ms() / 1e3, e.last_pack_ms() / 1e3))
        with tempfile.NamedTemporaryFile(suffix=".fq.gz") as f:
            f.write(data); f.flush()
            os.environ["CRASS_TIMING"] = "1"
            w, wl = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ix = ca.FastxIndex(f.name)
                w.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                e.lib.crass_hip_load_reads(e.h, ix.reads)
                wl.append(time.perf_counter() - t0)
                ix.close()
            os.environ.pop("CRASS_TIMING", None)
        say("(b) crass_index_fastx (host inflate side by side + parse + pack): wall %.3f s, + crass_hip_load_reads %.3f s" % (med(w), med(wl)))
    out.close()


if __name__ == "__main__":
    main()
