"""The comment kseq hands on from record to record, on the device (k_cm_bits / k_cm_tiles / k_cm_top, k_cm_source / k_cm_measure
/ k_span_copy) against the host function crass_fastx_comments_of on every designed job of tests/comment_sets.py, exact: the bytes,
the offsets and `has`.  Through crass_hip_load_fastx_files (plain files, and the same files as BGZF) — the first fetch builds the
structure on the arena — and through comments_build on caller-owned device bytes at every byte offset 0 .. 3; the _to form's
overflow rule with guard bytes around the buffer; CRASS_ERR_STATE after a drop and after a new load; the counters."""
import numpy as np
import pytest

from tests import bgzf_sets
from tests import comment_sets as cs

pytestmark = pytest.mark.gpu

JOBS = cs.jobs()
FILL = 0xA5
INVALID_ARG, STATE, OVERFLOW = 1, 6, 8
MIXED = ("every_third", "every_third_fq", "late_first", "long_comment", "sparse", "three_files", "open_end_between") + tuple("count_%d" % n for n in (63, 64, 65, 4095, 4096, 4097))


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


@pytest.fixture(scope="module")
def eng(ca):
    with ca.SearchEngine() as e:
        yield e


@pytest.fixture(scope="module")
def host(ca):
    """per job, computed once: (arena bytes, layout, (chars, off, has) of ALL records by the host function, own-comment records)"""
    out = {}
    for name, files in JOBS.items():
        lay = ca.fastx_files_scan_host(files)
        assert lay.accepted, name
        data = cs.arena(files)
        out[name] = (data, lay, ca.comments_of(data, lay.rec_pos, np.arange(lay.n_reads, dtype=np.uint64), lay.file_read_base),
                     sum(1 for m in cs.model(files) if m[2]))
    return out


def want_of(all_records, idx):
    chars, off, has = all_records
    items = [bytes(chars[int(off[r]):int(off[r + 1])]) for r in idx]
    c, o = cs.concat(items)
    return c, o, has[np.asarray(idx, np.int64)] if len(idx) else has[:0]


def lists(name, n):
    if name == "sparse":
        return [cs.SPARSE_QUERIES, cs.picks(name, n)[:3000]]
    return [list(range(n)), cs.picks(name, n)]


def check_fetch(eng, all_records, idx, what):
    want_c, want_o, want_h = want_of(all_records, idx)
    c, o, h = eng.fetch_comments(idx)
    assert np.array_equal(o, want_o), what
    assert np.array_equal(h, want_h), what
    assert np.array_equal(c[:int(want_o[-1])], want_c), what


def dev_bytes(data, lead=0, tail=64):
    """bytes in a device tensor that starts `lead` bytes behind an allocation, name bytes all around them"""
    import torch
    big = torch.full((len(data) + lead + tail,), 0x51, dtype=torch.uint8, device="cuda")
    t = big[lead:lead + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()))
    return big, t


@pytest.mark.parametrize("name", sorted(JOBS))
def test_files_load_then_fetch_equals_the_host_function(ca, eng, host, name):
    """plain files: the first fetch after the load builds the structure on the arena; the counters say what the set is"""
    data, lay, all_records, n_own = host[name]
    got = eng.load_fastx_files(JOBS[name])
    assert np.array_equal(got.rec_pos[:-1], lay.rec_pos[:-1]) and np.array_equal(got.file_read_base, lay.file_read_base), name
    for idx in lists(name, lay.n_reads):
        check_fetch(eng, all_records, idx, name)
    assert eng.comments_counters() == (n_own, lay.n_reads), name
    if name in MIXED:                                    # a set that really is mixed: some records have a comment of their own, some are handed one
        assert 0 < n_own < lay.n_reads and int(all_records[2].sum()) > n_own, name
    check_fetch(eng, all_records, [], name)


@pytest.mark.parametrize("name", ["every_third_fq", "crlf", "long_names", "count_4097", "sparse", "three_files", "open_end_between"])
def test_bgzf_files_load_then_fetch(ca, eng, host, name):
    """the same files as BGZF, inflated on the device into the arena (small blocks: several members per file)"""
    data, lay, all_records, n_own = host[name]
    eng.load_fastx_files([bgzf_sets.bgzf(f, block=3000) for f in JOBS[name]])
    for idx in lists(name, lay.n_reads):
        check_fetch(eng, all_records, idx, name)
    assert eng.comments_counters() == (n_own, lay.n_reads), name


@pytest.mark.parametrize("name", sorted(JOBS))
def test_caller_owned_bytes_equal_the_host_function(ca, eng, host, name):
    """comments_build on a device tensor of the caller's, at every byte offset 0 .. 3 of the bytes; no read set is needed"""
    data, lay, all_records, n_own = host[name]
    leads = range(4) if lay.n_reads < 1000 else (1,)
    for lead in leads:
        big, t = dev_bytes(data, lead)
        eng.comments_build(t, lay.rec_pos, lay.file_read_base)
        assert eng.comments_counters() == (n_own, lay.n_reads), (name, lead)
        for idx in lists(name, lay.n_reads):
            check_fetch(eng, all_records, idx, (name, lead))
    if lay.n_files == 1:                                 # file_read_base None: one file
        eng.comments_build(t, lay.rec_pos)
        check_fetch(eng, all_records, lists(name, lay.n_reads)[0], (name, "one file"))
    eng.comments_drop()


def test_more_tiles_than_one_step_of_the_carry_scan(ca, eng):
    """256 * 4096 + 4097 minimal records: 258 tiles, so the one block over the tiles' carries takes a second step, with the running
    maximum of the first in front.  Own comments only at record 0, at the last record of tile 255, at the first of tile 256 and
    at one record of the last tile; about 40 records on both sides of each are fetched (both sides of the boundary between the
    steps among them) and compared with crass_fastx_comments_of; the counters are the host's counts."""
    tile = 4096
    B = 256 * tile
    n = B + tile + 1
    own = {0: b"first", B - 1: b"end of tile 255", B: b"tile 256", n - 1: b"in the last tile"}
    assert (n - 1) // tile == 257 and len({len(c) for c in own.values()}) == len(own)
    recs = [b">x\n"] * n
    for r, c in own.items():
        recs[r] = b">x " + c + b"\n"
    data = b"".join(recs)
    rec_pos = np.zeros(n + 1, np.uint64)
    rec_pos[1:] = np.cumsum(np.fromiter(map(len, recs), np.uint64, n))
    assert int(rec_pos[-1]) == len(data)
    idx = sorted({r for p in own for r in range(max(p - 40, 0), min(p + 41, n))})
    idx = idx[::-1] + idx[::7]                           # out of order, with repeats
    want_c, want_o, want_h = ca.comments_of(data, rec_pos, idx)
    assert want_h.all() and bytes(want_c[:int(want_o[1])]) == own[n - 1]
    # the host's counts: every record is handed one of four comments of four lengths, each from where it starts
    all_o = ca.comments_of(data, rec_pos, np.arange(n, dtype=np.uint64))[1]
    handed = np.diff(all_o.astype(np.int64))
    starts = np.flatnonzero(np.diff(handed)) + 1
    assert starts.tolist() == sorted(own)[1:]
    big, t = dev_bytes(data, 3)
    eng.comments_build(t, rec_pos)
    assert eng.comments_counters() == (1 + len(starts), n)
    c, o, h = eng.fetch_comments(idx)
    assert np.array_equal(o, want_o) and np.array_equal(h, want_h) and np.array_equal(c[:int(want_o[-1])], want_c)
    eng.comments_drop()


def test_one_file_without_read_bases_carries_across_what_two_files_do_not(ca, eng, host):
    data, lay, all_records, _ = host["two_files"]
    big, t = dev_bytes(data)
    eng.comments_build(t, lay.rec_pos, lay.file_read_base)
    assert eng.fetch_comments(np.arange(20))[2].tolist() == [1] * 10 + [0] * 10
    eng.comments_build(t, lay.rec_pos)
    c, o, h = eng.fetch_comments(np.arange(20))
    wc, wo, wh = ca.comments_of(data, lay.rec_pos, np.arange(20))
    assert h.tolist() == [1] * 20 and np.array_equal(o, wo) and np.array_equal(c, wc)
    eng.comments_drop()


@pytest.mark.parametrize("name", ["every_third", "long_comment", "three_files", "count_4097"])
def test_to_form_overflow_rule(ca, eng, host, name):
    """into the caller's device buffer at every byte offset 0 .. 3: the capacity one short (status 8, offsets and has complete,
    nothing written), exact and one long; the bytes around the buffer keep their fill"""
    import torch
    data, lay, all_records, _ = host[name]
    eng.load_fastx_files(JOBS[name])
    idx = cs.picks(name, lay.n_reads)[:600]
    want_c, want_o, want_h = want_of(all_records, idx)
    total = int(want_o[-1])
    assert total > 1
    for lead, cap in ((0, total), (1, total - 1), (2, total + 1), (3, 0), (1, total)):
        big = torch.full((lead + cap + 16,), FILL, dtype=torch.uint8, device="cuda")
        out = big[lead:lead + cap]
        if cap < total:
            with pytest.raises(ca.CrassError) as err:
                eng.fetch_comments(idx, out=out)
            assert err.value.status == OVERFLOW, (name, cap)
            o, h, written = err.value.offsets, err.value.has, 0
        else:
            _, o, h = eng.fetch_comments(idx, out=out)
            written = total
        assert np.array_equal(o, want_o) and np.array_equal(h, want_h), (name, cap)
        got = big.cpu().numpy()
        assert np.array_equal(got[lead:lead + written], want_c[:written]), (name, cap)
        assert np.all(got[:lead] == FILL) and np.all(got[lead + written:] == FILL), (name, cap)
    # a NULL buffer of capacity 0 asks for the offsets alone; no bytes at all is fine
    lib = ca.load()
    ix = np.asarray(idx, np.uint64)
    off = np.zeros(len(ix) + 1, np.uint64)
    assert lib.crass_hip_fetch_comments_device_to(eng.h, ix.ctypes.data, len(ix), None, 0, off.ctypes.data, None) == OVERFLOW and np.array_equal(off, want_o)
    none = [r for r in range(lay.n_reads) if not all_records[2][r]][:3]
    if none:
        ix = np.asarray(none, np.uint64)
        assert lib.crass_hip_fetch_comments_device_to(eng.h, ix.ctypes.data, len(ix), None, 0, off.ctypes.data, None) == 0 and not off[:len(ix) + 1].any()
    # argument errors: nothing is written
    off[:] = 5
    assert lib.crass_hip_fetch_comments_device_to(eng.h, ix.ctypes.data, 1, None, 4, off.ctypes.data, None) == INVALID_ARG
    assert lib.crass_hip_fetch_comments_device_to(eng.h, ix.ctypes.data, 1, None, 0, None, None) == INVALID_ARG
    assert lib.crass_hip_fetch_comments_device_to(eng.h, None, 1, None, 0, off.ctypes.data, None) == INVALID_ARG
    bad = np.asarray([0, lay.n_reads], np.uint64)
    assert lib.crass_hip_fetch_comments_device_to(eng.h, bad.ctypes.data, 2, None, 0, off.ctypes.data, None) == INVALID_ARG and np.all(off == 5)
    with pytest.raises(ca.CrassError) as err:
        eng.fetch_comments([lay.n_reads])
    assert err.value.status == INVALID_ARG


def test_state_after_drop_and_after_a_new_load(ca, host):
    data, lay, all_records, n_own = host["every_third"]
    with ca.SearchEngine() as e:
        def refused(fn, *a, **kw):
            with pytest.raises(ca.CrassError) as err:
                fn(*a, **kw)
            return err.value.status
        import torch
        out = torch.zeros(64, dtype=torch.uint8, device="cuda")
        # a fresh context: nothing built, no arena
        assert refused(e.fetch_comments, [0]) == STATE and refused(e.fetch_comments, [0], out=out) == STATE and refused(e.comments_counters) == STATE
        assert refused(e.comments_build) == STATE        # (no arena to build on)
        big, t = dev_bytes(data)
        e.comments_build(t, lay.rec_pos, lay.file_read_base)
        check_fetch(e, all_records, [3, 4, 5], "built")
        e.comments_drop()
        assert refused(e.fetch_comments, [0]) == STATE and refused(e.fetch_comments, [0], out=out) == STATE and refused(e.comments_counters) == STATE
        e.comments_drop()                                # fine without one
        # a structure on caller-owned bytes goes with any load
        e.comments_build(t, lay.rec_pos, lay.file_read_base)
        e.load_text([b"ACGTACGTACGTACGTACGTACGTACGTACGT"] * 3)
        assert refused(e.fetch_comments, [0]) == STATE and refused(e.comments_counters) == STATE
        # a files load: the first fetch builds on the arena; the next load of another kind drops arena and structure
        e.load_fastx_files(JOBS["late_first"])
        assert refused(e.comments_counters) == STATE
        check_fetch(e, host["late_first"][2], [29, 0, 9, 8], "arena")
        assert e.comments_counters() == (host["late_first"][3], 30)
        e.load_fastx_files(JOBS["all"])                  # a new files load: the old structure is gone, the new set's is built by the fetch
        assert refused(e.comments_counters) == STATE
        check_fetch(e, host["all"][2], [29, 0], "arena 2")
        e.load_text([b"ACGTACGTACGTACGTACGTACGTACGTACGT"] * 3)
        assert refused(e.fetch_comments, [0]) == STATE and refused(e.fetch_comments, [0], out=out) == STATE
        # a failed build leaves what was there
        e.comments_build(t, lay.rec_pos, lay.file_read_base)
        far = lay.rec_pos.copy()
        far[4] = len(data)
        assert refused(e.comments_build, t, far, lay.file_read_base) == INVALID_ARG
        assert refused(e.comments_build, t, lay.rec_pos, [0, 5]) == INVALID_ARG
        check_fetch(e, all_records, list(range(30)), "kept")
        assert e.comments_counters() == (n_own, 30)
