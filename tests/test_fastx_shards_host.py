"""crass_fastx_files_shards_host — the cut rule of csrc/fastx_scan.h on the host, no GPU — against the brute-force statement of
tests/shard_sets.py: every byte position of each designed file as the nominal cut, 1 .. 7 ranks with even cuts, the records in
front of every cut against crass_fastx_files_scan_host's rec_pos, and the verdict of every declined input unchanged by any cut.
The serial probe (crass_fastx_cut_probe_host) and the pick of a record start from it, against the same brute force."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import files_sets, shard_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


DESIGNED = {"fastq": [shard_sets.small_fastq()], "fasta": [shard_sets.small_fasta()],
            "fasta_fastq": [shard_sets.small_fasta(), shard_sets.small_fastq()]}
DESIGNED.update({k: v[0] for k, v in shard_sets.cases().items() if not k.startswith("tile_edge") or k == "tile_edge_4096"})


def assert_rule(ca, files, n_ranks, nominal, what):
    sh = ca.fastx_files_shards_host(files, n_ranks, nominal)
    cuts, base = shard_sets.brute_shards(files, n_ranks, nominal)
    assert sh.accepted and sh.n_ranks == n_ranks and sh.n_files == len(files), what
    assert sh.cuts == cuts, (what, sh.cuts, cuts)
    assert sh.rank_read_base.tolist() == base, (what, sh.rank_read_base, base)
    return sh


@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_every_byte_as_the_nominal_cut_and_one_to_seven_ranks(ca, name):
    files = DESIGNED[name]
    T = shard_sets.text_bases(files)[-1]
    step = 1 if T < 2000 else 37                          # (the larger sets: every 37th byte and the designed positions)
    for x in sorted(set(range(0, T + 1, step)) | {T}):
        assert_rule(ca, files, 2, [x], (name, x))
    for n in range(1, 8):
        assert_rule(ca, files, n, None, (name, n))


@pytest.mark.parametrize("name", sorted(shard_sets.cases()))
def test_the_designed_positions(ca, name):
    files, positions = shard_sets.cases()[name]
    for n in (2, 3, 4):
        for nominal in shard_sets.nominal_lists(files, positions, n):
            assert_rule(ca, files, n, nominal, (name, n, nominal))


@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_rank_read_base_counts_the_records_in_front_of_each_cut(ca, name):
    files = DESIGNED[name]
    lay = ca.fastx_files_scan_host(files)
    assert lay.accepted
    tb = shard_sets.text_bases(files)
    # rec_pos are arena positions: a byte more per file in front
    rec_text = [int(p) - int(np.searchsorted(lay.file_byte_base, p, side="right") - 1) for p in lay.rec_pos[:-1]]
    for n in (2, 3, 5):
        sh = ca.fastx_files_shards_host(files, n)
        assert sh.n_reads == lay.n_reads and sh.max_len == lay.max_len and sh.formats == lay.formats
        assert np.array_equal(sh.file_read_base, lay.file_read_base)
        for g, (f, p) in enumerate(sh.cuts):
            x = tb[f] + p if f < len(files) else tb[-1]
            assert int(sh.rank_read_base[g]) == sum(1 for r in rec_text if r < x), (name, n, g)


def test_the_designed_sets_are_what_they_say():
    fq, fa = shard_sets.small_fastq(), shard_sets.small_fasta()
    assert 150 < len(fq) < 300 and 150 < len(fa) < 300
    assert b"\n@IIIIII\n" in fq and b"\n+IIIIIII\n" in fq            # quality lines that start with '@' and '+'
    assert any(len(rec.split(b"\n")) > 3 for rec in fa.split(b">")[1:])      # multi-line records
    cuts, base = shard_sets.brute_shards([b">short\nACGT\n>long\n" + b"A" * 500 + b"\n"], 4)
    assert len(set(cuts)) < len(cuts)                                  # an empty rank


DECLINED = dict({k: v for k, v in shard_sets.declined().items()},
                **{k: (v[0], [None]) for k, v in files_sets.declined().items()})


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_a_declined_input_keeps_its_verdict_for_every_cut(ca, name):
    files, positions = DECLINED[name]
    want = ca.fastx_files_scan_host(files)
    assert not want.accepted
    small = sum(len(f) for f in files) < 2000
    T = sum(len(f) for f in files)
    sweeps = [[x] for x in range(T + 1)] if small else []
    for n, nominal in [(2, s) for s in sweeps] + [(n, None) for n in range(1, 8)]:
        try:
            sh = ca.fastx_files_shards_host(files, n, nominal)
        except ca.CrassError as e:                                    # (a cut beyond the text of the files in front of the decline)
            assert e.status == 1 and nominal is not None
            continue
        assert not sh.accepted and sh.verdict == want.verdict, (name, n, nominal, sh.verdict, want.verdict)
        assert len(sh.rank_read_base) == 0 and len(sh.cut_pos) == 0
    if name == "fastq_header_lacks_at_on_the_cut":
        assert want.decline_reason == 4
    if name == "incomplete_last_record":
        assert want.decline_reason == 3 and want.decline_pos == files[0].rindex(b"@q5")
    if name == "lone_header_at_the_end":
        assert want.decline_reason == 10


def test_the_serial_probe_and_the_pick(ca):
    none = (1 << 64) - 1
    for text in (shard_sets.small_fastq(), shard_sets.small_fasta()):
        starts = shard_sets.record_starts(text)
        for a in range(len(text)):
            for b in sorted({a, a + 1, a + 17, len(text)}):
                if b > len(text):
                    continue
                left = a == 0 or text[a - 1:a] == b"\n"
                out = ca.fastx_cut_probe_host(text[a:b], left)
                ls = [p - a for p in range(a, b) if p == 0 or text[p - 1:p] == b"\n"]
                assert int(out[0]) == text[a:b].count(b"\n") and int(out[1]) == min(4, len(ls))
                assert [int(v) for v in out[2:6]] == (ls + [none] * 4)[:4]
                gt = [p for p in ls if text[a + p] == 0x3E]
                assert int(out[6]) == (gt[0] if gt else none)
                # the pick (fx_probe_pick, restated): FASTA the first '>' line start; FASTQ the first of the four whose index is 0 mod 4
                if text[:1] == b">":
                    pick = int(out[6])
                else:
                    first_idx = text[:a].count(b"\n") + (0 if left else 1)
                    k = (-first_idx) % 4
                    pick = int(out[2 + k]) if k < int(out[1]) else none
                want = [s for s in starts if a <= s < b]
                if pick != none or not want:
                    assert pick == (want[0] - a if want else none), (a, b)
                else:                                                 # (more than four line starts in front of it: never in a range that holds one)
                    raise AssertionError((a, b, want))


def test_invalid_arguments(ca):
    fq = shard_sets.small_fastq()
    for n, nominal in ((0, None), (65, None), (3, [10, 5]), (2, [len(fq) + 1])):
        with pytest.raises((ca.CrassError, ValueError)) as e:
            ca.fastx_files_shards_host([fq], n, nominal)
        assert not isinstance(e.value, ca.CrassError) or e.value.status == 1


def test_member_rule_program(tmp_path):
    """tools/sanitize/shards_main.cpp without a file: the self-check of the host arithmetic of a rank's shard (csrc/fastx_shards.h,
    csrc/fastx_scan.cpp) under AddressSanitizer + UBSan, as a stand-alone program with the sanitizer runtimes linked statically and
    nothing preloaded.  bgzf_members_for over every tiling it enumerates or draws (fixed seed; indices of 1 .. 8 members of 0, 1,
    2, 5 or 16 bytes, up to three inner cuts): every range enclosed by its members and every member taken by some range, no case
    failing; shard_stage_place over designed pieces: phase, no overlap, the buffer's size."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "shards_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "crass_amd", "csrc", "fastx_scan.cpp"), os.path.join(ROOT, "crass_amd", "csrc", "bgzf.cpp"),
                           os.path.join(ROOT, "tools", "sanitize", "shards_main.cpp"), "-o", exe])
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[0].startswith("ok   member rule:") and lines[0].endswith(" 0 fail"), lines
    assert int(lines[0].split()[3]) >= 100000, lines[0]      # tilings checked
    assert lines[1].startswith("ok   placement:") and lines[-1] == "ok  : 0 failures", lines
    assert not any(w in r.stderr for w in ("runtime error", "AddressSanitizer", "LeakSanitizer")), r.stderr[-3000:]


HOST_READER = ("ingest", "fastx_parse", "host_inflate", "fastx_read", "fastx_index", "fastx_stream", "synth", "pgzip")


def test_host_reader_program(tmp_path):
    """tools/sanitize/ingest_main.cpp over the files of the host reader (csrc/ingest.cpp and the six beside it, csrc/pgzip.cpp)
    under AddressSanitizer + UBSan, as a stand-alone program with the sanitizer runtimes linked statically and nothing preloaded:
    FASTA and FASTQ, each plain, wrapped, with CRLF line ends, without a final newline, truncated and with a record that has no
    comment behind ones that have (the stale buffers), and each of those gzip'd, read by the whole-file reader, the stream and the
    index in pieces of 200 bytes.  Exit status 0, an `ok` line per file with the records and bases tests/fastx.py reads from
    it, no sanitizer report.  (The objects are compiled side by side and without optimisation: one -O1 -g run over all of them
    is more than 20 s.)"""
    import gzip
    from tests import fastx
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-std=c++17", "-O0", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
             "-I" + os.path.join(ROOT, "include")]
    srcs = [os.path.join(ROOT, "crass_amd", "csrc", s + ".cpp") for s in HOST_READER] + [os.path.join(ROOT, "tools", "sanitize", "ingest_main.cpp")]
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs]
    jobs = [subprocess.Popen([cxx] + flags + ["-c", s, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for s, o in zip(srcs, objs)]
    for s, j in zip(srcs, jobs):
        msg = j.communicate()[0]
        assert j.returncode == 0, (s, msg[-3000:])
    exe = str(tmp_path / "ingest_asan")
    subprocess.check_call([cxx] + flags + objs + ["-o", exe, "-lz", "-ldl", "-lpthread"])

    def seq(i):
        return "".join("ACGT"[(i * 7 + k * k + k // 3) % 4] for k in range(20 + (i * 37) % 90)) if i % 11 else "ACGNNT" * 5

    def fasta(eol="\n", wrap=0):
        body = lambda s: eol.join(s[k:k + wrap] for k in range(0, len(s), wrap)) if wrap else s
        return "".join(">r%d%s%s%s%s" % (i % 23, " c%d" % i if i % 3 else "", eol, body(seq(i)), eol) for i in range(40))

    def fastq(eol="\n", wrap=0, comments=True):
        body = lambda s: eol.join(s[k:k + wrap] for k in range(0, len(s), wrap)) if wrap else s
        return "".join("@q%d%s%s%s%s+%s%s%s" % (i, " c%d" % i if comments or i < 20 else "", eol, body(seq(i)), eol, eol,
                                               body("".join("I5#@+>~"[(i + k) % 7] for k in range(len(seq(i))))), eol) for i in range(40))

    texts = {}
    for kind, make in (("fa", fasta), ("fq", fastq)):
        plain = make()
        texts[kind + "_plain"] = plain
        texts[kind + "_wrapped"] = make(wrap=17)
        texts[kind + "_crlf"] = make(eol="\r\n")
        texts[kind + "_no_final_newline"] = plain[:-1]
        texts[kind + "_truncated"] = plain[:len(plain) * 2 // 3 + 5]
    texts["fa_no_comments"] = "".join(">n%d\n%s\n" % (i, seq(i)) for i in range(40))
    texts["fq_stale_comments"] = fastq(comments=False)
    assert len(texts) == 12
    paths = []
    for name, t in sorted(texts.items()):
        for suffix, data in ((".txt", t.encode()), (".gz", gzip.compress(t.encode(), 6))):
            paths.append(str(tmp_path / (name + suffix)))
            with open(paths[-1], "wb") as f:
                f.write(data)
    env = dict(os.environ, CRASS_FASTX_CHUNK="200", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(paths), lines
    for p, line in zip(paths, lines):
        recs = fastx.read_fastx(p[:p.rindex(".")] + ".gz")         # (the helper opens its input through gzip)
        want = "ok   %s: whole rc 0, %d records %d bases; " % (p, len(recs), sum(len(x[2]) for x in recs))
        assert line.startswith(want), (line, want)
    assert not any(w in r.stderr for w in ("runtime error", "AddressSanitizer", "LeakSanitizer")), r.stderr[-3000:]
