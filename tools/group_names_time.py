#!/usr/bin/env python3
"""What the found-name exchange of a group step costs on either route (crass_hip_group_set_name_exchange), measured, not gated.

Two paired FASTQ files (R1 / R2: the two mates of a pair carry the same name) of --reads / 2 synthetic 150 bp reads each
(default 2 x 2 M), loaded with crass_hip_group_load_fastx_files into groups of 2 and of 4 CONTEXTS SHARING ONE GPU (local copies).
Per group: one warm-up step on each route, then --reps (5) steps on each, ALTERNATING host / device in one session.  Per step:
the exchange part — names_publish .. names_lookup, the barrier between them included — as wall time and as HIP-event time on the
rank's stream (crass_hip_group_name_exchange_ms; the slowest rank), and the wall time of the whole step beside them.  Medians.

Contexts that share one GPU say nothing about peer copies between real devices: here every copy between "ranks" is a copy inside
one device's memory.  Output: stdout and profiles/NOTES_r22.md (--out)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["CRASS_GROUP_NAMES_TIMING"] = "1"        # (read when a group is created: the two events around the exchange)
import numpy as np
import torch        # noqa: F401  (before the library: one HIP runtime in the process, torch's)
import crass_amd as ca
from tools.load_files_time import fastq_bytes

ca.load()
OUT = None


def say(text):
    print(text, flush=True)
    if OUT:
        OUT.write(text + "\n")
        OUT.flush()


def med(v):
    return float(np.median(v))


def mate(first, n, L, name_first):
    """fastq_bytes(first, n, L) under the names of the reads name_first .. name_first + n: the other mate's file"""
    rec = np.frombuffer(fastq_bytes(first, n, L), np.uint8).reshape(n, -1).copy()
    idx = np.arange(name_first, name_first + n, dtype=np.int64)
    for d in range(8):
        rec[:, 8 - d] = ord("0") + (idx // 10 ** d) % 10
    return rec.tobytes()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "NOTES_r22.md"))
    a = ap.parse_args()
    OUT = open(a.out, "w")
    half = a.reads // 2
    say("# The found-name exchange of a group step, host route against device route: measured once, medians of %d\n" % a.reps)
    files = [np.frombuffer(fastq_bytes(0, half, a.len), np.uint8), np.frombuffer(mate(half, half, a.len, 0), np.uint8)]
    say("Two paired FASTQ files (every name once in each), %d reads of %d bp each, %.3f GB of text.  Steps alternate between the" % (half, a.len, sum(len(f) for f in files) / 1e9))
    say("routes in one session; exchange = names_publish .. names_lookup with the barrier between them, the slowest rank's.\n")
    say("| contexts on one GPU | route | names published | namesakes found | exchange wall ms | exchange HIP-event ms | step wall ms |")
    say("|---|---|---|---|---|---|---|")
    for n in (2, 4):
        with ca.SearchGroup([0] * n, local_copies=True) as g:
            g.load_fastx_files(files)
            rows = {0: [], 1: []}
            counts = {}
            for rep in range(a.reps + 1):              # (rep 0: the warm-up of each route — first-call bounds, buffers)
                for route in (0, 1):
                    g.set_name_exchange(bool(route))
                    t0 = time.perf_counter()
                    g.step()
                    step_ms = 1e3 * (time.perf_counter() - t0)
                    ms = [g.name_exchange_ms(r) for r in range(n)]
                    cnt = [g.name_exchange_counters(r) for r in range(n)]
                    assert all(c[0] == route for c in cnt), cnt
                    counts[route] = (sum(c[1] for c in cnt), sum(c[3] for c in cnt))
                    if rep:
                        rows[route].append((max(m[0] for m in ms), max(m[1] for m in ms), step_ms))
            assert counts[0] == counts[1], counts
            for route in (0, 1):
                v = np.asarray(rows[route])
                say("| %d | %s | %d | %d | %.3f | %.3f | %.3f |" % (n, ("host", "device")[route], counts[route][0], counts[route][1],
                                                                 med(v[:, 0]), med(v[:, 1]), med(v[:, 2])))
    say("\nThe contexts of every row share one device, its memory, its copy engines and one host: a copy between two \"ranks\" is a copy")
    say("inside one device's memory.  The rows say what either route costs there; they say nothing about peer copies between real")
    say("devices (hipMemcpyPeerAsync over the fabric), which a one-GPU box cannot measure.  The default route stays the host's.")
    OUT.close()


if __name__ == "__main__":
    main()
