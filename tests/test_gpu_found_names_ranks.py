"""The found-header exchange of the one-process-per-GPU launcher (crass_amd.distributed.FoundNameExchange) end to end: two gloo
processes share the one GPU, rank r holds FASTQ file r's bytes on the device, and the two files hold mates with the SAME name.
readsFound is keyed by the name (libcrispr.cpp:138,411): a mate whose partner was found in pass 1 — on whichever rank — is not
recruited in pass 2.  With the exchange the two ranks' records together equal the oracle's on the concatenation with the shared
names, record for record; without it they equal the oracle's with unique names, which is what the launcher did before."""
import json
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import fastx_sets, orc
from tests.parity import assert_same_pipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, N_FILE, PAIRS, N_DR, FREE = 150, 2000, 120, 8, 40


def design(seed):
    """two files of N_FILE reads of L bases.  For pair k both files hold a record named pair<k>: one mate carries three copies of
    a direct repeat of 24 bases with spacers of 30 .. 38 bases, at least one base from either end of the read (found in pass 1), the other exactly one copy in random background
    (recruitable in pass 2 only).  The found mate lies in file 0 for even k, in file 1 for odd k.  FREE reads per file carry one
    copy under a name of their own; everything else is random reads with names of their own.  Returns (names[2], seqs[2], singles[2]: the record numbers of the one-copy mates per file)."""
    rng = random.Random(seed)
    acgt = lambda n: fastx_sets.acgt(rng, n)

    def edged(n, first, last):
        x = bytearray(acgt(n))
        if first is not None:
            x[0] = first
        if last is not None:
            x[-1] = last
        return bytes(x)

    drs = [acgt(24) for _ in range(N_DR)]
    names = [[b"filler%d_%d" % (f, i) for i in range(N_FILE)] for f in range(2)]
    seqs = [[acgt(L) for _ in range(N_FILE)] for _ in range(2)]
    slots = [rng.sample(range(N_FILE), PAIRS + FREE) for _ in range(2)]
    for f in range(2):                                    # one-copy reads with names of their own: recruited whatever the mates do
        for j, at_rec in enumerate(slots[f][PAIRS:]):
            dr, at = drs[j % N_DR], rng.randint(0, L - 24)
            seqs[f][at_rec] = acgt(at) + dr + acgt(L - 24 - at)
    singles = [[], []]
    for k in range(PAIRS):
        dr = drs[k % N_DR]
        s1, s2 = rng.randint(30, 38), rng.randint(30, 38)
        # (the bases in front of the three copies differ from one another, and so do those behind them: the repeat is not
        # extended into its spacers, which would make spacers of 30 bases too short for pass 1)
        before, behind = rng.sample(b"ACGT", 3), rng.sample(b"ACGT", 3)
        left = rng.randint(1, L - (72 + s1 + s2) - 1)
        found = edged(left, None, before[0]) + dr + edged(s1, behind[0], before[1]) + dr + edged(s2, behind[1], before[2]) + dr
        found += edged(L - len(found), behind[2], None)
        assert len(found) == L
        at = rng.randint(0, L - len(dr))
        single = acgt(at) + dr + acgt(L - len(dr) - at)
        f_found = k % 2
        for f, s in ((f_found, found), (1 - f_found, single)):
            names[f][slots[f][k]] = b"pair%d" % k
            seqs[f][slots[f][k]] = s
        singles[1 - f_found].append(slots[1 - f_found][k])
    return names, seqs, singles


def fastq(names, seqs, f):
    return b"".join(fastx_sets.fq(nm + b" mate %d" % (f + 1), s) for nm, s in zip(names, seqs))


WORKER = r"""
import os, sys, json
sys.path.insert(0, %(root)r)
import numpy as np
import torch, torch.distributed as dist
import crass_amd as ca
from crass_amd.distributed import allgather_distinct, FoundNameExchange
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group(backend="gloo", rank=rank, world_size=world)
data = open(%(file)r %% rank, "rb").read()
base = %(n_file)d * rank
t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
eng = ca.SearchEngine(device=0)
lay = eng.attach_device_fastx(t, pad_uniform=2, read_index_base=base)
assert lay.n_reads == %(n_file)d
eng.device_header_ids(t, lay, install=True)              # the local header ids
eng.names_build(t, lay)
xf = FoundNameExchange(eng, dist, read_index_base=base)

def run(exchange):
    cand = eng.seed_scan()
    chars, lens, cmap = eng.distinct()
    g_chars, g_lens, my_off = allgather_distinct(chars, lens, dist)
    eng.merge_distinct(g_chars, g_lens, my_off)
    extra = xf.extra_found(cand.read_idx - np.uint64(base), t, lay, build=False) if exchange else None
    rec = eng.recruit(extra_found=extra)
    m = eng.merge_view()
    return dict(read=cand.read_idx.tolist(), low=cand.low_lexi.tolist(), replen=cand.repeat_len.tolist(),
                ss=[cand.ss(k) for k in range(cand.n)], tok=m.cand_token[:cand.n].tolist(),
                r_read=rec.read_idx.tolist(), r_low=rec.low_lexi.tolist(), r_ss=[[int(a), int(b)] for a, b in zip(rec.start, rec.end)],
                r_tok=rec.token.tolist(), tokens=[x.decode() for x in m.tokens], groups=m.groups,
                patterns=[p.decode() for p in m.patterns], pat_group=[int(g) for g in m.pat_group],
                extra=[] if extra is None else [int(x) for x in extra])

out = dict(control=run(False), exchange=run(True))
json.dump(out, open(%(out)r %% rank, "w"))
eng.close()
dist.destroy_process_group()
"""


class Joined:
    """the two ranks' records as one result with the fields tests/parity.py reads: rank order == read order"""

    def __init__(self, r):
        cat = lambda k: r[0][k] + r[1][k]
        assert r[0]["tokens"] == r[1]["tokens"] and r[0]["groups"] == r[1]["groups"]
        assert r[0]["patterns"] == r[1]["patterns"] and r[0]["pat_group"] == r[1]["pat_group"]
        self.n_pass1, self.n_pass2 = len(cat("read")), len(cat("r_read"))
        self.rec_read = np.asarray(cat("read") + cat("r_read"), np.uint64)
        self.rec_lowlexi = np.asarray(cat("low") + cat("r_low"), np.uint8)
        self.rec_replen = np.asarray(cat("replen") + [0] * self.n_pass2, np.uint32)
        self._ss = cat("ss") + cat("r_ss")
        self.rec_nss = np.asarray([len(s) for s in self._ss], np.uint32)
        self.rec_token = np.asarray(cat("tok") + cat("r_tok"), np.uint32)
        self.tokens = [t.encode() for t in r[0]["tokens"]]
        self.groups, self.n_groups, self.n_tokens = r[0]["groups"], len(r[0]["groups"]), len(self.tokens)
        self.patterns = [p.encode() for p in r[0]["patterns"]]
        self.pat_group, self.n_patterns = r[0]["pat_group"], len(self.patterns)

    def ss(self, k):
        return self._ss[k]


def pass2_reads(res):
    return res.rec_read[res.n_pass1:res.n_pass1 + res.n_pass2].tolist()


def test_two_ranks_with_shared_names_equal_the_oracle(tmp_path):
    names, seqs, singles = design(20)
    all_seqs = seqs[0] + seqs[1]
    shared = orc.pipeline(all_seqs, headers=names[0] + names[1])
    unique = orc.pipeline(all_seqs, headers=[b"u%d" % i for i in range(2 * N_FILE)])
    # the input tests something, from the oracle alone: the shared names keep (nearly) every designed one-copy mate out of pass 2,
    # in both directions (file 0's mates found in file 1, and the reverse)
    kept_out = set(pass2_reads(unique)) - set(pass2_reads(shared))
    assert set(pass2_reads(shared)) <= set(pass2_reads(unique))
    designed = [set(singles[0]), set(N_FILE + s for s in singles[1])]
    assert len(designed[0]) == len(designed[1]) == PAIRS // 2
    for f in range(2):
        lo, hi = f * N_FILE, (f + 1) * N_FILE
        more = sum(1 for x in pass2_reads(unique) if lo <= x < hi) - sum(1 for x in pass2_reads(shared) if lo <= x < hi)
        assert more >= 0.9 * len(designed[f]), (f, more)
    assert kept_out <= designed[0] | designed[1]
    assert shared.n_pass2 >= 0.9 * 2 * FREE and shared.n_pass1 >= 0.9 * PAIRS and np.array_equal(shared.rec_read[:shared.n_pass1], unique.rec_read[:unique.n_pass1])

    for f in range(2):
        (tmp_path / ("file%d.fq" % f)).write_bytes(fastq(names[f], seqs[f], f))
    outpat = str(tmp_path / "rank%d.json")
    script = tmp_path / "worker.py"
    script.write_text(WORKER % dict(root=ROOT, file=str(tmp_path / "file%d.fq"), n_file=N_FILE, out=outpat))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    r = [json.load(open(outpat % k)) for k in range(2)]
    # with the exchange: the oracle on the concatenation with the shared names, record for record
    assert_same_pipeline(Joined([r[0]["exchange"], r[1]["exchange"]]), shared)
    # every rank was told of the other's found names, as LOCAL record numbers of its own mates
    for f in range(2):
        found_here = set(shared.rec_read[:shared.n_pass1].tolist())
        told = set(f * N_FILE + x for x in r[f]["exchange"]["extra"])
        assert told and told <= designed[f] and kept_out & designed[f] <= told
        assert not told & found_here
    # the control, what the launcher did before: every name its own, and so exactly those reads more
    control = Joined([r[0]["control"], r[1]["control"]])
    assert_same_pipeline(control, unique)
    assert set(pass2_reads(control)) - set(pass2_reads(shared)) == kept_out and kept_out
