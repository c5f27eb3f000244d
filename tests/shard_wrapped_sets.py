"""The cut rule of csrc/fastx_scan.h for FASTQ class 1 (record-aligned shards of wrapped FASTQ files) stated by brute force,
and the designed inputs of tests/test_fastx_shards_class_host.py, tests/test_gpu_group_wrapped_files.py and
tools/sanitize/shards_class_dump.py.

Under class 1 the record starts of a file whose byte 0 is '@' are the header lines of the records the wrapped rule walks from
line 0 — wrapped_sets.judge(text)[2] —, and nothing else: a quality line may start with '@' and the lines behind it may parse as
a complete record.  FASTA files keep shard_sets.record_starts.  The actual cut is the smallest record start at or after the
nominal one, or T.  Generated data only; everything is deterministic."""
import bisect
import random

from tests import bgzf_sets, files_sets, shard_sets, wrapped_sets
from tests.fastx_sets import acgt, filler_fq, fq

TILE = shard_sets.TILE

# A quality line that is a decoy: the bytes from "@dec" on parse ON THEIR OWN as a valid chain of three records, none of which
# is one of the file's.
DECOY = (b"@r0 c\nACGTACGTAC\nGGTT\n+\nIIIIIIIIII\nIIII\n"
         b"@r1\nACGTACGTACGTA\n+\n@dec\nACGT\n+\nIIII\n"
         b"@r2\nTT\nGG\n\n+r2\nII\nII\n\n\n"
         b"@r3\nACG\n+\n@II")
DECOY_STARTS, DECOY_AT = [0, 40, 77, 100, 113], 60


def record_starts(text):
    if text[:1] != b"@":
        return shard_sets.record_starts(text)
    reason, _, rec_pos, _ = wrapped_sets.judge(text)
    assert reason == 0, reason
    return rec_pos[:-1]


def brute_shards(files, n_ranks, nominal=None):
    """-> (cuts [(file, pos)] * (n_ranks + 1), rank_read_base [n_ranks + 1]), as shard_sets.brute_shards"""
    texts = files_sets.text_of(files)
    tb = shard_sets.text_bases(files)
    T = tb[-1]
    starts = [tb[f] + p for f, t in enumerate(texts) for p in record_starts(t)]
    nominal = shard_sets.default_nominal(files, n_ranks) if nominal is None else list(nominal)
    cuts, base = [], []
    for x in [0] + nominal + [T]:
        k = bisect.bisect_left(starts, x)
        base.append(k)
        if k == len(starts):
            cuts.append((len(files), 0))
        else:
            f = bisect.bisect_right(tb, starts[k]) - 1
            cuts.append((f, starts[k] - tb[f]))
    return cuts, base


def second_small():
    """about 150 bytes: quality lines that start with '@' and '+', an empty-sequence record, CRLF, void lines, no final '\\n'"""
    return (b"@s0 c0\r\nACGT\r\nAC\r\n+s0\r\n@II\r\n+II\r\n\r\n"
            b"@e\n+\n\n \n"
            b"@s1\nTTTTGGGGCC\n+\n@s9\n+\nIIIIII\n\t\n"
            b"@s2 c2\nA\nC\nG\n+\n+\n@\nI\n"
            b"@s3\nGATTACAGATTACA\n+\n@IIIIIIIIIIIII\n\n\n"
            b"@s4\nAC\n+\n@I")


def edge_file(target):
    """a wrapped file one of whose records starts at byte `target`: four-line filler in front, wrapped records behind"""
    rng = random.Random("shard_wrapped_sets:edge:%d" % target)
    rec = wrapped_sets.wfq(b"edge", acgt(rng, 90), (b"@+I" * 30), w=30)
    tail = b"".join(wrapped_sets.wfq(b"t%d" % i, acgt(rng, 20 + i), (b"@I+" * 20)[:20 + i], w=7, after=(b"",) if i % 2 else ()) for i in range(6))
    return wrapped_sets.at_offset(rec, 0, target, tail)


def around(text, marks, reach=1):
    out = set()
    for m in marks:
        out.update(range(max(0, m - reach), min(len(text), m + reach) + 1))
    return sorted(out)


def cases():
    """name -> (files, positions, files the wrapped rule cuts); every position is to be a nominal cut of some rank (text space),
    None stands for the even cuts.  Every job holds a file outside the four-line class, so a class-1 load takes two attempts."""
    rng = random.Random("shard_wrapped_sets:cases")
    D = wrapped_sets.designed(TILE)
    out = {}
    out["decoy"] = ([DECOY], [None, 41, 59, 60, 61, 77, 78, 112], 1)
    q = D["quality_starts_with_at_and_plus"]
    at = [i + 1 for i in range(len(q) - 1) if q[i:i + 1] == b"\n" and q[i + 1:i + 2] in (b"@", b"+")]
    out["quality_starts_with_at_and_plus"] = ([q], [None] + at[1:9], 1)
    e = D["empty_then_void"]
    out["empty_sequence_record"] = ([e], [None] + around(e, [e.index(b"@e\n"), e.index(b"@e2")]), 1)
    c = D["crlf"]
    cr = c.index(b"\r\n", 100)
    out["crlf"] = ([c], [None, cr, cr + 1, cr + 2] + around(c, [c.index(b"@r3")]), 1)
    v = D["void_lines"]
    out["void_lines_at_the_cut"] = ([v], [None] + around(v, [v.index(b"\n\r\n") + 1, v.index(b"\n  \n") + 1, v.index(b"\x80\xff"), len(v) - 3], 2)[:16], 1)
    nf = D["no_final_newline"]
    out["last_line_without_newline"] = ([second_small(), nf], [None, len(second_small()) - 2, len(second_small()) - 1, len(second_small()), len(second_small()) + len(nf) - 1,
                                                                len(second_small()) + len(nf)], 2)
    lg = D["read_9000_wrap60"]
    out["record_longer_than_a_range"] = ([lg], [None, 100, 3000, 6000, 9300, 12000, 15000, len(lg) - 30, len(lg) - 5], 1)
    out["more_ranks_than_records"] = ([D["one_base"], D["empty_only"]], [None, 1, 5, 9, 10, 12], 2)
    for target in (TILE - 1, TILE, TILE + 1):
        f = edge_file(target)
        assert target in record_starts(f)
        out["record_start_at_%d" % target] = ([f], [None] + list(range(target - 2, target + 3)) + [10, 2 * TILE], 1)
    big = wrapped_sets.n_records(1025)
    assert big.count(b"\n") > 4 * 1024
    out["more_than_1024_lines"] = ([big], [None, 4095, 4096, 4097, 8192, 12288, len(big) - 10], 1)
    fa, four = shard_sets.small_fasta(), shard_sets.small_fastq()
    mixed = [DECOY + b"\n", fa, four, bgzf_sets.bgzf(second_small(), block=70)]
    b0, b1, b2 = len(mixed[0]), len(mixed[0]) + len(fa), len(mixed[0]) + len(fa) + len(four)
    out["mixed_job"] = (mixed, [None, 50, b0, b0 + 60, b1, b1 + 100, b2, b2 + 1, b2 + 69, b2 + 70, b2 + 71, b2 + 140, b2 + 200], 3)
    return out


def declined():
    """name -> (files, positions): every offending input wrapped_sets names, on its own and behind an accepted wrapped file;
    cuts at, before and behind the offence"""
    out = {}
    for name, (data, reason, pos) in wrapped_sets.declines(TILE).items():
        T = len(data)
        out[name] = ([data], [None] + sorted({min(T, max(0, p)) for p in (pos - 1, pos, pos + 1, T // 3, T - 2)}))
        if data:
            n0 = len(DECOY) + 1
            out["behind_decoy_" + name] = ([DECOY + b"\n", data], [None] + sorted({min(n0 + T, max(0, p)) for p in (45, n0, n0 + pos, n0 + pos + 1, n0 + T - 1)}))
    return out


def four_line_job():
    """inside the four-line class: a class-1 load takes one attempt"""
    rng = random.Random("shard_wrapped_sets:four")
    return [b"".join(fq(b"f%d" % i, acgt(rng, 30 + i), bytes(rng.choices(b"@+I5", k=30 + i))) for i in range(12)), shard_sets.small_fasta(), filler_fq(300)]


def nominal_lists(files, positions, n_ranks):
    return shard_sets.nominal_lists(files, positions, n_ranks)
