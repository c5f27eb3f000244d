"""Several input files into one resident set on the device (crass_hip_load_fastx_files) against the host restatement
(crass_fastx_files_scan_host), the host packer on the joined text (crass_pack_reads) and the host route (crass_index_fastx_files +
crass_hip_load_reads); file, record and quality-line edges on scan tile and vector edges; declined sets; the same answers through
seed scan, merge and recruit; the quality strings of records from the arena (crass_hip_fetch_quality_device).  Every comparison is
exact equality."""
import gzip
import os

import numpy as np
import pytest

from tests import files_sets

pytestmark = pytest.mark.gpu

T = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("packed", "word_off", "lengths", "exc_read", "exc_off", "exc_bytes")
SCALARS = ("n_reads", "stride_words", "uniform_len", "n_exceptions", "read_index_base")
ACCEPTED = files_sets.accepted()
EDGE = files_sets.edge_sets(T)
DECLINED = files_sets.declined()
SETS = dict(ACCEPTED, **EDGE)


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    assert crass_amd.load().crass_hip_fastx_tile_bytes() == T
    return crass_amd


@pytest.fixture(scope="module")
def eng(ca):
    with ca.SearchEngine() as e:
        yield e


def assert_same_set(got, want, what, arrays=ARRAYS):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in arrays:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            if not np.array_equal(got[k], want[k]):
                bad = np.flatnonzero(got[k] != want[k])
                raise AssertionError("%s: %s differs at %d places, first %d: %r != %r" % (what, k, len(bad), bad[0], got[k][bad[0]], want[k][bad[0]]))


def ids_of(arrays):
    return np.arange(arrays["n_reads"], dtype=np.uint64) if arrays["header_id"] is None else arrays["header_id"]


def assert_same_layout(lay, host, what):
    assert lay.accepted and host.accepted and lay.verdict == host.verdict, what
    assert (lay.n_files, lay.n_reads, lay.max_len, lay.formats) == (host.n_files, host.n_reads, host.max_len, host.formats), what
    for k in ("file_read_base", "file_byte_base", "rec_pos", "seq_off"):
        assert np.array_equal(getattr(lay, k), getattr(host, k)), (what, k)


@pytest.mark.parametrize("name", sorted(SETS))
def test_resident_set_equals_the_host_routes(ca, eng, name, tmp_path):
    files = SETS[name]
    host = ca.engine.fastx_files_scan_host(files)
    arena, reads = files_sets.joined(files, host.rec_pos)
    hid = ca.fastx_header_ids(arena, host.rec_pos)
    for pad in (2, 0, 1):
        lay = eng.load_fastx_files(files, pad_uniform=pad)
        assert_same_layout(lay, host, (name, pad))
        pk = ca.PackedReads(reads, pad_uniform=pad)
        want = ca.packed_arrays(pk.reads)
        res = eng.packed()
        got = res.arrays()
        assert_same_set(got, want, (name, pad))
        assert np.all(got["packed"][-4:] == 0)
        assert np.array_equal(ids_of(got), hid), (name, pad)
        cnt = eng.counters()
        assert cnt["n_reads"] == want["n_reads"] and cnt["n_exceptions"] == want["n_exceptions"], (name, pad)
        assert cnt["bytes_reads_device"] == 4 * (len(want["packed"]) - 4), (name, pad)
        res.close()
        pk.close()
        addr, nb = eng.resident_fastx()
        assert addr and nb == len(arena) == int(host.file_byte_base[-1])
    # the host route itself: crass_index_fastx_files on the files on disk + crass_hip_load_reads (its packer's mode is 2)
    ix = ca.engine.FastxIndex(files_sets.write_files(files, tmp_path))
    lay = eng.load_fastx_files(files, pad_uniform=2)
    res = eng.packed()
    got = res.arrays()
    res.close()
    with ca.SearchEngine() as other:
        other.load_reads(ix)
        res = other.packed()
        want = res.arrays()
        res.close()
        # (the index's own packer gives the bytes of an exception read that are not A C G T another code than crass_pack_reads'
        # 0 — the search reads such reads from the exception list —, so the words are compared with crass_pack_reads above and
        # everything else with the index here)
        assert_same_set(got, want, (name, "index"), [k for k in ARRAYS if k != "packed"])
        assert got["packed"].shape == want["packed"].shape
        clean = np.ones(len(got["packed"]), bool)
        if got["stride_words"]:
            for r in got["exc_read"]:
                clean[int(r) * got["stride_words"]:(int(r) + 1) * got["stride_words"]] = False
        else:
            for r in got["exc_read"]:
                clean[int(got["word_off"][int(r)]):int(got["word_off"][int(r) + 1])] = False
        assert np.array_equal(got["packed"][clean], want["packed"][clean]), (name, "index")
        assert np.array_equal(ids_of(got), ids_of(want)), name
        for k in ("n_reads", "n_exceptions", "bytes_reads_device"):
            assert eng.counters()[k] == other.counters()[k], (name, k)
    assert lay.max_len == ix.max_len
    ix.close()


def test_the_edge_sets_are_what_they_say(ca):
    bases = set()
    for name, files in EDGE.items():
        host = ca.engine.fastx_files_scan_host(files)
        assert host.accepted, name
        bases.update(int(b) % 16 for b in host.file_byte_base[:-1])
        arena = b"".join(t + b"\n" for t in files_sets.text_of(files))
        part = name.split("_")
        if part[0] in ("record", "quality") and part[1] == "on":
            modulus, b1 = int(part[2]), int(host.file_byte_base[1])
            r = int(host.file_read_base[1]) + 45
            pos = int(host.rec_pos[r])
            if part[0] == "quality":
                for _ in range(3):
                    pos = arena.index(b"\n", pos) + 1
            assert (b1 % 16 + pos - b1) % modulus == 0 and pos - b1 > T, name      # (the file's tiles start at its base rounded down to 16)
    assert bases == set(range(16))
    assert len(EDGE["file_ends_on_tile_edge"][0]) == T and len(EDGE["file_starts_on_tile_edge"][0]) + 1 == T
    assert len(EDGE["tiny_first_file"][0]) < T
    assert ACCEPTED["plain_bgzf"][1].endswith(files_sets.bgzf_sets.EOF) and len(files_sets.bgzf_sets.EOF) == 28


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_sets(ca, eng, name):
    files, want = DECLINED[name]
    host = ca.engine.fastx_files_scan_host(files)
    assert files_sets.verdict_of(host) == want
    eng.load_fastx_files(ACCEPTED["one_file"])                   # something is resident, and an arena kept
    with pytest.raises(ca.engine.FastxFilesDeclined) as e:
        eng.load_fastx_files(files)
    assert e.value.status == 2 and e.value.layout.verdict == host.verdict and files_sets.verdict_of(e.value.layout) == want
    assert len(e.value.layout.rec_pos) == 0 and e.value.layout.n_reads == 0
    with pytest.raises(ca.CrassError) as e:                      # no reads resident, as after a failed crass_hip_load_text
        eng.seed_scan()
    assert e.value.status == 6
    with pytest.raises(ca.CrassError) as e:
        eng.resident_fastx()
    assert e.value.status == 6
    lay = eng.load_fastx_files(ACCEPTED["fasta_fastq"])          # the context is as good as new
    assert_same_layout(lay, ca.engine.fastx_files_scan_host(ACCEPTED["fasta_fastq"]), name)
    eng.seed_scan()
    assert eng.resident_fastx()[1] == int(lay.file_byte_base[-1])


def test_a_read_beyond_the_length_limit_is_declined_with_its_file(ca, eng):
    long = b">long\n" + b"ACGT" * 20000 + b"\n"                  # 80 000 bases
    first = ACCEPTED["one_file"][0]
    with pytest.raises(ca.engine.FastxFilesDeclined) as e:
        eng.load_fastx_files([first, b">ok\nACGT\n" + long])
    lay = e.value.layout
    assert (lay.decline_file, lay.decline_reason, lay.decline_pos, lay.bgzf[0]) == (1, 11, len(b">ok\nACGT\n"), 0)


def test_another_load_lets_the_arena_go(ca, eng):
    eng.load_fastx_files(ACCEPTED["fasta_fastq"])
    assert eng.resident_fastx()[1] > 0
    eng.load_text([b"ACGTACGT", b"GGGG"])
    with pytest.raises(ca.CrassError) as e:
        eng.resident_fastx()
    assert e.value.status == 6


def test_invalid_arguments(ca, eng):
    import ctypes as C
    from crass_amd import _abi
    lib = ca.load()
    v = _abi.FastxFilesLayoutC()
    assert lib.crass_hip_load_fastx_files(eng.h, None, None, 0, 2, C.byref(v)) == 1
    a = np.frombuffer(b">a\nACGT\n", np.uint8)
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    lens = np.array([len(a)], np.uint64)
    assert lib.crass_hip_load_fastx_files(eng.h, ptrs, lens.ctypes.data_as(_abi.u64p), 1, 3, C.byref(v)) == 1
    assert lib.crass_hip_load_fastx_files(None, ptrs, lens.ctypes.data_as(_abi.u64p), 1, 2, C.byref(v)) == 1
    assert lib.crass_hip_load_fastx_files(eng.h, ptrs, lens.ctypes.data_as(_abi.u64p), 1, 2, None) == 0      # (out may be NULL)


# ---- the same answers through the path ----
def run_path(e):
    return e.seed_scan(), e.merge(), e.recruit()


def assert_same_fields(a, b, what):
    assert type(a) is type(b)
    keys = sorted(k for k in vars(a) if not k.startswith("_"))
    assert keys == sorted(k for k in vars(b) if not k.startswith("_")) and keys, what
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)
        else:
            assert x == y, (what, k)


def two_files_from_golden(ca):
    """the regression input CN_gDC twice: as it is, and with every second record renamed — the other half of the second file's
    headers repeat the first file's; the second file BGZF-compressed"""
    text = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "data", "CN_gDC.fa.gz"), "rb").read())
    lay = ca.fastx_scan_host(text)
    assert lay.accepted and lay.n_reads > 1000
    recs = [text[int(lay.rec_pos[r]):int(lay.rec_pos[r + 1])] for r in range(lay.n_reads)]
    second = b"".join(rec if r % 2 == 0 else rec[:1] + b"mate_" + rec[1:] for r, rec in enumerate(recs))
    return [text, files_sets.bgzf_sets.bgzf(second, block=60000)]


def test_same_answers_through_the_path(ca, tmp_path):
    files = two_files_from_golden(ca)
    ix = ca.engine.FastxIndex(files_sets.write_files(files, tmp_path))
    with ca.SearchEngine() as a, ca.SearchEngine() as b, ca.SearchEngine() as plain:
        lay = a.load_fastx_files(files, pad_uniform=2)
        b.load_reads(ix)
        n1 = int(lay.file_read_base[1])
        res = a.packed()
        hid = ids_of(res.arrays())
        res.close()
        assert lay.n_reads == 2 * n1 == ix.n_reads
        res = b.packed()
        assert np.array_equal(hid, ids_of(res.arrays()))
        res.close()
        assert np.all(hid[n1::2] < n1) and np.all(hid[n1 + 1::2] >= n1)      # every second header of the second file repeats one of the first
        ra, rb = run_path(a), run_path(b)
        for x, y, part in zip(ra, rb, ("candidates", "merge", "recruits")):
            assert_same_fields(x, y, part)
        for k in ("n_reads", "n_exceptions", "n_pass1_found", "n_pass2_found", "n_patterns", "bytes_reads_device", "used_fast_filter"):
            assert a.counters()[k] == b.counters()[k], k
        # a header repeated across the two files is skipped in pass 2: without header ids more reads are recruited
        plain.load_fastx_files(files, pad_uniform=2)
        plain.set_header_ids(None)
        rp = run_path(plain)
        assert ra[0].n > 0 and ra[1].n_patterns > 0 and rp[2].n > 0
        found = set(int(hid[int(i)]) for i in ra[0].read_idx)
        assert not any(int(hid[int(i)]) in found for i in ra[2].read_idx)
    ix.close()


# ---- quality strings from the arena ----
QUAL_SETS = {"fastq_fasta_bgzf": [ACCEPTED["one_file"][0], ACCEPTED["fasta_fastq"][0], files_sets.bgzf_sets.bgzf(ACCEPTED["crlf"][1], block=3000)],
             "quality_on_4096_lead5": EDGE["quality_on_4096_lead5"], "quality_on_16_lead15": EDGE["quality_on_16_lead15"],
             "no_final_newline": ACCEPTED["no_final_newline"], "empty_read": ACCEPTED["empty_read"]}


def index_lists(n):
    rng = np.random.default_rng(3)
    return {"all": np.arange(n), "none": np.zeros(0, np.int64), "every_7th": np.arange(0, n, 7),
            "descending_with_repeats": np.concatenate([np.arange(n - 1, -1, -3), [0, 0, n - 1, n - 1], rng.integers(0, n, 20)])}


@pytest.mark.parametrize("name", sorted(QUAL_SETS))
def test_quality_strings(ca, eng, name, tmp_path):
    import torch
    files = QUAL_SETS[name]
    lay = eng.load_fastx_files(files)
    addr, nb = eng.resident_fastx()
    ix = ca.engine.FastxIndex(files_sets.write_files(files, tmp_path))
    arena = b"".join(t + b"\n" for t in files_sets.text_of(files))
    for what, idx in index_lists(lay.n_reads).items():
        recs = ix.fetch(idx) if len(idx) else []
        want = [r[3] for r in recs]                              # crass_fastx_index_fetch's qual (None: has_qual 0)
        assert want == [files_sets.quality_of(arena, lay.rec_pos, int(r)) for r in idx], (name, what)
        chars, off, has = eng.fetch_quality(addr, nb, lay.rec_pos, idx)
        assert len(off) == len(idx) + 1 and off[0] == 0 and has.tolist() == [0 if w is None else 1 for w in want], (name, what)
        got = [chars[int(off[k]):int(off[k + 1])].tobytes() for k in range(len(idx))]
        assert got == [w or b"" for w in want], (name, what)
        # into a device buffer between two guard bands
        total, guard = int(off[-1]), 64
        for lead in (0, 3):
            buf = torch.full((guard + lead + total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
            out = buf[guard + lead:guard + lead + total]
            none, off2, has2 = eng.fetch_quality(addr, nb, lay.rec_pos, idx, out=out)
            back = buf.cpu().numpy()
            assert none is None and np.array_equal(off2, off) and np.array_equal(has2, has), (name, what)
            assert back[guard + lead:guard + lead + total].tobytes() == chars.tobytes(), (name, what, lead)
            assert np.all(back[:guard + lead] == 0xA5) and np.all(back[guard + lead + total:] == 0xA5), (name, what, lead)
        if total:
            small = torch.full((total - 1,), 0xA5, dtype=torch.uint8, device="cuda")
            with pytest.raises(ca.CrassError) as e:
                eng.fetch_quality(addr, nb, lay.rec_pos, idx, out=small)
            assert e.value.status == 8 and np.array_equal(e.value.offsets, off) and np.all(small.cpu().numpy() == 0xA5)
    ix.close()


def test_quality_of_a_line_with_blanks_inside(ca, eng):
    """the quality string is the line's bytes 33..126: blanks inside the line are none of it (the copy walks such a line)"""
    fq = b"@a\nACGT\n+\nI I\tII\n@b\nAC\n+\n#$\r\n@c\n\n+\n\n"
    lay = eng.load_fastx_files([fq])
    addr, nb = eng.resident_fastx()
    chars, off, has = eng.fetch_quality(addr, nb, lay.rec_pos, [2, 0, 1, 0])
    assert [chars[int(off[k]):int(off[k + 1])].tobytes() for k in range(4)] == [b"", b"IIII", b"#$", b"IIII"] and has.tolist() == [1, 1, 1, 1]


def test_quality_argument_checks(ca, eng):
    import ctypes as C
    from crass_amd import _abi
    lay = eng.load_fastx_files(ACCEPTED["fasta_fastq"])
    addr, nb = eng.resident_fastx()
    chars, off, has = eng.fetch_quality(addr, nb, lay.rec_pos, [])      # n == 0: CRASS_OK, nothing
    assert len(chars) == 0 and off.tolist() == [0] and len(has) == 0
    rp = lay.rec_pos.copy()
    rp[5] = nb                                                   # a record position beyond the arena: refused on the host
    with pytest.raises(ca.CrassError) as e:
        eng.fetch_quality(addr, nb, rp, [4, 5])
    assert e.value.status == 1
    with pytest.raises(ca.CrassError) as e:
        eng.fetch_quality(addr, nb, lay.rec_pos, [lay.n_reads])
    assert e.value.status == 1
    v = _abi.Text()
    idx = np.zeros(1, np.uint64)
    assert ca.load().crass_hip_fetch_quality_device(eng.h, addr, nb, lay.rec_pos.ctypes.data, lay.n_reads, idx.ctypes.data, 1, None, None) == 1
    assert ca.load().crass_hip_fetch_quality_device(None, addr, nb, lay.rec_pos.ctypes.data, lay.n_reads, idx.ctypes.data, 1, C.byref(v), None) == 1
    assert ca.load().crass_hip_fetch_quality_device(eng.h, addr, nb, lay.rec_pos.ctypes.data, lay.n_reads, None, 1, C.byref(v), None) == 1
    # the header lines and the header ids work on the arena unchanged
    arena = b"".join(t + b"\n" for t in files_sets.text_of(ACCEPTED["fasta_fastq"]))
    rp = np.append(lay.rec_pos[:-1], np.uint64(nb))
    ids, n_rep = eng.device_header_ids(addr, rp, install=False)
    assert np.array_equal(ids, ca.fastx_header_ids(arena, lay.rec_pos))
    pick = [0, lay.n_reads - 1, int(lay.file_read_base[1]) - 1, int(lay.file_read_base[1])]
    lines, loff, name_len = eng.fetch_header_lines(addr, rp, pick)
    for k, r in enumerate(pick):
        p = int(lay.rec_pos[r])
        assert lines[int(loff[k]):int(loff[k + 1])].tobytes() == arena[p + 1:arena.index(b"\n", p)], r
