#!/usr/bin/env python3
"""What it costs to inflate a plain (single-member) gzip FASTQ on the device chunk by chunk (gunzip.hip), against the host's
several-thread inflate of the same file (pgzip.cpp inside the indexed reader).

One input held in memory (and written once to a scratch file for the reader that takes a path): a synthetic four-line FASTQ of
150 bp reads, --text-gb (default 1.0) of text, one gzip member at zlib level 6.  Median of --reps (3), one process:
  (a) SearchEngine.inflate_gzip_device at chunk sizes 64 / 128 / 256 / 512 KB, the compressed bytes already in HBM: wall seconds
      of the whole call (header, find, count, chain, decode, windows, narrow, CRC) and with timing level 1 the event times of the
      five kernels (crass_hip_last_gzip_ms), the find kernel's share of their sum, and the chain's shape
  (b) SearchEngine.load_fastx_gzip (default chunk size): wall seconds from host bytes to resident packed reads, and its parts
  (c) crass_index_fastx on the same .gz: the host's several-thread inflate + parse + pack (CRASS_TIMING=1 prints its stage times
      to stderr), then crass_hip_load_reads
  (d) SearchEngine.inflate_gzip_members_device (members mode, default chunk size) on the same text as ONE member and as 16 members
      of equal text size: wall seconds, the five event times (narrow's includes k_gz_member_crc and the round trip in front of
      it), the chain's shape and the number of members
Output: stdout and profiles/gunzip_mi355x.txt (--out)."""
import argparse
import os
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import crass_amd as ca
from tools.inflate_time import make_text, med

ca.load()
STEPS = ("find", "count", "decode", "windows", "narrow")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-gb", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gunzip_mi355x.txt"))
    a = ap.parse_args()
    out = open(a.out, "w")

    def say(t):
        print(t, flush=True)
        out.write(t + "\n")
        out.flush()

    text = make_text(int(a.text_gb * 1e9))
    t0 = time.perf_counter()
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    data = b"".join(co.compress(text[at:at + (64 << 20)]) for at in range(0, len(text), 64 << 20)) + co.flush()
    say("text %.3f GB, gzip %.3f GB (%.2f x), compressed in %.1f s" % (len(text) / 1e9, len(data) / 1e9, len(text) / len(data), time.perf_counter() - t0))
    arr = np.frombuffer(data, np.uint8).copy()
    with ca.SearchEngine() as e:
        e.set_stage_timing(1)
        d_in = torch.from_numpy(arr).to("cuda")
        d_out = torch.empty(len(text), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        best = None
        for kb in (64, 128, 256, 512):
            n, plan = e.inflate_gzip_device(d_in, d_out, kb << 10, with_plan=True)      # warm: allocations, code objects
            assert n == len(text)
            wall, parts = [], {k: [] for k in STEPS}
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.inflate_gzip_device(d_in, d_out, kb << 10)
                wall.append(time.perf_counter() - t0)
                for k, v in e.last_gzip_ms().items():
                    parts[k].append(v / 1e3)
            kern = sum(med(parts[k]) for k in STEPS)
            say("(a) chunk %3d KB: %d chunks, %d on the chain; wall %.3f s (%.2f GB of text per second); kernels %.3f s = %s; find is %.0f %% of them" %
                (kb, plan.n_chunks, plan.n_chain, med(wall), len(text) / 1e9 / med(wall), kern,
                 " + ".join("%s %.3f" % (k, med(parts[k])) for k in STEPS), 100 * med(parts["find"]) / kern))
            if best is None or med(wall) < best[1]:
                best = (kb, med(wall))
        say("    fastest: %d KB" % best[0])
        assert bytes(d_out[:1 << 20].cpu().numpy()) == text[:1 << 20] and bytes(d_out[-(1 << 20):].cpu().numpy()) == text[-(1 << 20):]
        # (d) members mode: the file above as it is, and the same text cut into 16 members
        per = (len(text) + 15) // 16
        def member(t):
            co = zlib.compressobj(6, zlib.DEFLATED, 31)
            return co.compress(t) + co.flush()
        sixteen = b"".join(member(text[at:at + per]) for at in range(0, len(text), per))
        for label, blob in (("1 member", None), ("16 members", sixteen)):
            d_m = d_in if blob is None else torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to("cuda")
            n, plan, members = e.inflate_gzip_members_device(d_m, d_out, 0, with_plan=True)      # warm
            assert n == len(text)
            wall, parts = [], {k: [] for k in STEPS}
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.inflate_gzip_members_device(d_m, d_out, 0)
                wall.append(time.perf_counter() - t0)
                for k, v in e.last_gzip_ms().items():
                    parts[k].append(v / 1e3)
            say("(d) members mode, %s: %d chunks, %d on the chain, %d members; wall %.3f s (%.2f GB of text per second); kernels %s" %
                (label, plan.n_chunks, plan.n_chain, members.n_members, med(wall), len(text) / 1e9 / med(wall),
                 " + ".join("%s %.3f" % (k, med(parts[k])) for k in STEPS)))
            assert bytes(d_out[:1 << 20].cpu().numpy()) == text[:1 << 20] and bytes(d_out[-(1 << 20):].cpu().numpy()) == text[-(1 << 20):]
            del d_m
        del d_in, d_out
        torch.cuda.empty_cache()
        e.load_fastx_gzip(arr)
        wall, infl, scan, pack = [], [], [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lay = e.load_fastx_gzip(arr)
            wall.append(time.perf_counter() - t0)
            infl.append(e.last_inflate_ms() / 1e3); scan.append(e.last_scan_ms() / 1e3); pack.append(e.last_pack_ms() / 1e3)
        say("(b) load_fastx_gzip (default chunk): wall %.3f s, of it inflate kernels %.3f + scan %.3f + pack %.3f (+ upload, chain, waits); %d reads" %
            (med(wall), med(infl), med(scan), med(pack), lay.n_reads))
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
        say("(c) crass_index_fastx (host several-thread inflate + parse + pack): wall %.3f s, + crass_hip_load_reads %.3f s" % (med(w), med(wl)))
    out.close()


if __name__ == "__main__":
    main()
