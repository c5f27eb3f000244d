"""Sequence text packed on the device (crass_hip_load_text / crass_hip_attach_device_text, pack.hip) against the host
route (crass_pack_reads + crass_hip_load_reads): the resident set bit for bit (crass_hip_get_packed), the same answers
through seed scan, merge and recruit, the error codes, and the adapter's CRASS_DEVICE_PACK switch.  Every comparison
is exact equality."""
import os
import subprocess

import numpy as np
import pytest

from tests import text_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
ARRAYS = ("packed", "word_off", "lengths", "exc_read", "exc_off", "exc_bytes", "header_id")
SCALARS = ("n_reads", "stride_words", "uniform_len", "n_exceptions", "read_index_base")


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


_sets = {}


def get_set(ca, name):
    if name not in _sets:
        seqs = text_sets.make(ca, name)
        _sets[name] = (seqs,) + text_sets.concat(seqs)
    return _sets[name]


def assert_same_set(got, want, what):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            if not np.array_equal(got[k], want[k]):
                bad = np.flatnonzero(got[k] != want[k])
                raise AssertionError("%s: %s differs at %d places, first %d: %r != %r" % (what, k, len(bad), bad[0], got[k][bad[0]], want[k][bad[0]]))
    assert np.all(want["packed"][-4:] == 0) and np.all(got["packed"][-4:] == 0)


def engine_with_chunk(ca, chunk):
    old = os.environ.pop("CRASS_TEXT_CHUNK_BYTES", None)
    if chunk:
        os.environ["CRASS_TEXT_CHUNK_BYTES"] = str(chunk)
    try:
        return ca.SearchEngine()                          # (the switch is read when the context is created)
    finally:
        os.environ.pop("CRASS_TEXT_CHUNK_BYTES", None)
        if old is not None:
            os.environ["CRASS_TEXT_CHUNK_BYTES"] = old


def host_reference(ca, buf, off, pad):
    pk = ca.PackedReads((buf, off), pad_uniform=pad)
    want = ca.packed_arrays(pk.reads)
    pk.close()
    return want


def check_both_routes(ca, eng, buf, off, pad, what):
    import torch
    want = host_reference(ca, buf, off, pad)
    eng.load_text((buf, off), pad_uniform=pad)
    res = eng.packed()
    assert_same_set(res.arrays(), want, what + " load_text")
    cnt = eng.counters()
    assert cnt["n_reads"] == want["n_reads"] and cnt["n_exceptions"] == want["n_exceptions"]
    assert cnt["bytes_reads_device"] == 4 * (len(want["packed"]) - 4)
    res.close()
    t = torch.from_numpy(buf).to("cuda") if len(buf) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    eng.attach_device_text(t, off, pad_uniform=pad)
    t.fill_(0x4E)                                        # the context kept nothing of the text: overwrite it, then let it go
    torch.cuda.synchronize()
    del t
    torch.cuda.empty_cache()
    junk = torch.full((max(len(buf), 1),), 0x47, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = eng.packed()
    assert_same_set(res.arrays(), want, what + " attach_device_text")
    assert eng.counters()["n_exceptions"] == want["n_exceptions"]
    res.close()
    del junk


# ---- 1. bit equality of the resident set ----
@pytest.mark.parametrize("name", text_sets.LAYOUT_SETS)
def test_resident_set_is_the_host_packers(ca, name):
    seqs, buf, off = get_set(ca, name)
    with engine_with_chunk(ca, 0) as eng:
        for pad in (0, 1, 2):
            check_both_routes(ca, eng, buf, off, pad, "%s pad %d" % (name, pad))


@pytest.mark.parametrize("name", text_sets.LAYOUT_SETS)
def test_resident_set_in_many_chunks(ca, name):
    """every input again with the host text in at least five chunks (a seventh of the text per chunk), in chunks smaller than
    the longest read (one read per chunk then) and in 37-byte chunks — chunk ends inside shared output vectors, exception
    reads first and last in a chunk.  Sets of fewer than five reads cannot make five chunks: they take the values as they
    come.  The 100 k set takes 4 096 bytes for its smallest chunk (37 bytes would be 100 000 launches)."""
    seqs, buf, off = get_set(ca, name)
    longest = max((len(s) for s in seqs), default=0)
    small = 4096 if len(seqs) > 20000 else 37
    for chunk in (max(1, len(buf) // 7), max(1, longest - 1), small):
        if len(seqs) >= 5:
            n_chunks, at = 0, 0                           # the chunks the engine's rule makes: whole reads, at least one each
            while at < len(seqs):
                end = at + 1
                while end < len(seqs) and int(off[end + 1] - off[at]) <= max(chunk, longest, 1):
                    end += 1
                at, n_chunks = end, n_chunks + 1
            assert n_chunks >= 5, (name, chunk, n_chunks)
        with engine_with_chunk(ca, chunk) as eng:
            for pad in (0, 1, 2):
                want = host_reference(ca, buf, off, pad)
                eng.load_text((buf, off), pad_uniform=pad)
                res = eng.packed()
                assert_same_set(res.arrays(), want, "%s pad %d chunk %d" % (name, pad, chunk))
                res.close()


@pytest.mark.parametrize("name", ["uniform150", "ragged", "odd_bytes"])
def test_text_starting_mid_buffer_at_an_odd_address(ca, name):
    """offsets whose first entry is not 0: the text starts 13 (77) bytes into the buffer, behind bytes that are not bases"""
    import torch
    seqs, buf, off = get_set(ca, name)
    for lead in (13, 77):
        buf2 = np.concatenate([np.full(lead, 0x4E, np.uint8), buf, np.full(5, 0x6E, np.uint8)])
        off2 = off + np.uint64(lead)
        for chunk in (0, max(1, len(buf) // 6)):
            with engine_with_chunk(ca, chunk) as eng:
                for pad in (0, 2):
                    want = host_reference(ca, buf, off, pad)
                    assert_same_set(host_reference(ca, buf2, off2, pad), want, "host packer, shifted text")
                    eng.load_text((buf2, off2), pad_uniform=pad)
                    res = eng.packed()
                    assert_same_set(res.arrays(), want, "%s lead %d chunk %d load_text" % (name, lead, chunk))
                    res.close()
                    big = torch.from_numpy(buf2).to("cuda")
                    eng.attach_device_text(big, off2, pad_uniform=pad)
                    res = eng.packed()
                    assert_same_set(res.arrays(), want, "%s lead %d attach_device_text" % (name, lead))
                    res.close()
                    odd = torch.empty(len(buf2) + 3, dtype=torch.uint8, device="cuda")[3:]      # the tensor itself at an odd address
                    odd.copy_(big)
                    assert odd.data_ptr() % 2 == 1
                    eng.attach_device_text(odd, off2, pad_uniform=pad)
                    res = eng.packed()
                    assert_same_set(res.arrays(), want, "%s lead %d attach_device_text (odd tensor)" % (name, lead))
                    res.close()


def test_packed_after_load_reads_and_header_ids(ca):
    """crass_hip_get_packed after the host route gives back what was loaded, header ids and index base included"""
    seqs, buf, off = get_set(ca, "trimmed")
    hid = np.arange(len(seqs), dtype=np.uint64)
    hid[100:200] = 7
    for pad in (0, 2):
        pk = ca.PackedReads((buf, off), pad_uniform=pad)
        want = ca.packed_arrays(pk.reads)
        want["header_id"], want["read_index_base"] = hid, 12345
        with ca.SearchEngine() as eng:
            eng.load_reads(pk, header_id=hid, read_index_base=12345)
            res = eng.packed()
            assert_same_set(res.arrays(), want, "load_reads pad %d" % pad)
            res.close()
            eng.load_text((buf, off), pad_uniform=pad, header_id=hid, read_index_base=12345)
            res = eng.packed()
            assert_same_set(res.arrays(), want, "load_text pad %d" % pad)
            res.close()


# ---- 2. the same answers through the path ----
def run_path(eng):
    cand = eng.seed_scan()
    mer = eng.merge()
    rec = eng.recruit()
    return cand, mer, rec


def assert_same_fields(a, b, what):
    # tests/parity.py's one helper compares a PipelineResult with the oracle's; here two engines' CandidateSet / MergeResult /
    # RecruitSet are compared with each other, field by field.  This relies on those classes keeping every result field as a
    # public instance attribute (crass_amd/engine.py): the key list below is checked to be the same and not empty.
    assert type(a) is type(b)
    keys = sorted(k for k in vars(a) if not k.startswith("_"))
    assert keys == sorted(k for k in vars(b) if not k.startswith("_")) and keys, what
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)
        else:
            assert x == y, (what, k)


def assert_same_path(ca, buf, off, pad, what, header_id=None, base=0, min_found=1):
    with ca.SearchEngine() as a, ca.SearchEngine() as b:
        a.load_text((buf, off), pad_uniform=pad, header_id=header_id, read_index_base=base)
        pk = ca.PackedReads((buf, off), pad_uniform=pad)
        b.load_reads(pk, header_id=header_id, read_index_base=base)
        ra, rb = run_path(a), run_path(b)
        for x, y, part in zip(ra, rb, ("candidates", "merge", "recruits")):
            assert_same_fields(x, y, what + " " + part)
        for k in ("n_reads", "n_exceptions", "n_pass1_found", "n_pass2_found", "n_patterns", "bytes_reads_device", "used_fast_filter"):
            assert a.counters()[k] == b.counters()[k], (what, k)
        assert ra[0].n >= min_found, what
        if base:
            assert ra[0].n and int(ra[0].read_idx.min()) >= base
        return ra


def test_same_answers_synthetic(ca):
    seqs, buf, off = get_set(ca, "synth100k")
    for pad in (0, 2):
        cand, mer, rec = assert_same_path(ca, buf, off, pad, "synthetic pad %d" % pad, min_found=100)
        assert rec.n > 0 and mer.n_patterns > 0


def test_same_answers_with_header_ids_and_index_base(ca):
    seqs, buf, off = get_set(ca, "synth100k")
    hid = np.arange(len(seqs), dtype=np.uint64)
    hid[1::2] = hid[0::2]                                # mates share a header: a pass-1 hit of one keeps the other out of pass 2
    assert_same_path(ca, buf, off, 2, "synthetic, header ids, index base", header_id=hid, base=5_000_000, min_found=100)


@pytest.mark.parametrize("fname", sorted(os.listdir(DATA)))
def test_same_answers_regression_inputs(ca, fname):
    f = ca.FastxFile(os.path.join(DATA, fname))
    hid = None if f.unique_headers() else f.header_id
    assert_same_path(ca, f.seq, f.seq_off, 2, fname, header_id=hid, min_found=0)


def test_same_answers_ragged_long_reads_with_n(ca):
    import random
    rng = random.Random(99)
    drs = [bytes(rng.choices(b"ACGT", k=rng.randint(28, 37))) for _ in range(6)]
    seqs = []
    for i in range(600):
        L = rng.randint(300, 5000)
        if i % 4 == 0:                                   # an array: repeats of one DR with random spacers, inside random flanks
            dr = drs[i % len(drs)]
            body = b"".join(dr + bytes(rng.choices(b"ACGT", k=rng.randint(30, 38))) for _ in range(rng.randint(3, 12)))
            pre = bytes(rng.choices(b"ACGT", k=rng.randint(0, 200)))
            s = (pre + body + bytes(rng.choices(b"ACGT", k=max(0, L - len(pre) - len(body)))))[:5000]
        else:
            s = bytes(rng.choices(b"ACGT", k=L))
        if i % 7 == 0:
            s = text_sets.with_n(rng, s, 2)
        seqs.append(s)
    buf, off = text_sets.concat(seqs)
    cand, mer, rec = assert_same_path(ca, buf, off, 2, "ragged long reads", min_found=50)
    exc = {i for i, s in enumerate(seqs) if set(s) - set(b"ACGT")}
    assert exc & set(cand.read_idx.tolist()), "no exception read among the candidates: the case does not cover them"


# ---- 3. errors ----
def test_errors(ca):
    import ctypes as C
    import torch
    lib = ca.load()
    with ca.SearchEngine() as eng:
        with pytest.raises(ca.CrassError) as e:
            eng.packed()
        assert e.value.status == 6                       # CRASS_ERR_STATE: no reads yet
        seqs, buf, off = get_set(ca, "uniform150")
        eng.load_text((buf, off))
        eng.seed_scan()
        long_buf = np.frombuffer(b"ACGT" * 15026, dtype=np.uint8).copy()
        long_off = np.array([0, 100, 60101, 60104], dtype=np.uint64)      # the middle read has 60 001 bases
        dev = torch.from_numpy(long_buf).to("cuda")
        for call in (lambda: eng.load_text((long_buf, long_off)), lambda: eng.attach_device_text(dev, long_off)):
            eng.load_text((buf, off))
            with pytest.raises(ca.CrassError) as e:
                call()
            assert e.value.status == 2                   # CRASS_ERR_UNSUPPORTED
            with pytest.raises(ca.CrassError) as e:
                eng.seed_scan()
            assert e.value.status == 6                   # ... and the reads loaded before are gone
            with pytest.raises(ca.CrassError) as e:
                eng.packed()
            assert e.value.status == 6
        ok_off = np.array([0, 100, 60100, 60104], dtype=np.uint64)        # 60 000 bases: the limit itself is taken
        eng.load_text((long_buf, ok_off))
        res = eng.packed()
        assert_same_set(res.arrays(), host_reference(ca, long_buf, ok_off, 2), "60 000-base read")
        res.close()
        dec = np.array([0, 150, 100, 300], dtype=np.uint64)
        for call in (lambda: eng.load_text((buf, dec)), lambda: eng.attach_device_text(dev, dec)):
            with pytest.raises(ca.CrassError) as e:
                call()
            assert e.value.status == 1                   # CRASS_ERR_INVALID_ARG
        for fn in (lib.crass_hip_load_text, lib.crass_hip_attach_device_text):
            assert fn(eng.h, None, off.ctypes.data, 3, 2, None, 0) == 1
            assert fn(eng.h, int(dev.data_ptr()), None, 3, 2, None, 0) == 1
            assert fn(eng.h, int(dev.data_ptr()), off.ctypes.data, 3, 3, None, 0) == 1       # pad_uniform outside 0 .. 2
            assert fn(None, None, None, 0, 2, None, 0) == 1
            assert fn(eng.h, None, None, 0, 2, None, 0) == 0                                 # no reads: fine
            res = eng.packed()
            assert res.n_reads == 0 and res.arrays()["packed"].tolist() == [0, 0, 0, 0]
            res.close()
        assert lib.crass_hip_get_packed(eng.h, None) == 1


# ---- 4. the adapter ----
@pytest.mark.parametrize("fname", ["CN_gDC.fa.gz", "Ill100.fx.gz"])
def test_adapter_device_pack_writes_the_same_files(ca, tmp_path, fname):
    """crass-hip over the whole-file ingest route with CRASS_DEVICE_PACK=1 (the reader's text goes to crass_hip_load_text)
    against the same run without the switch: every output file byte for byte"""
    from crass_amd import build
    cli = build.build_adapter()
    path = os.path.join(DATA, fname)
    import shutil
    outs = {}
    d = tmp_path / "out"
    for tag, extra in (("host", {}), ("device", {"CRASS_DEVICE_PACK": "1"})):      # the same command in the same place, one after the other
        d.mkdir()
        env = dict(os.environ, CRASS_INGEST="whole", CRASS_TIMING="1")
        env.pop("CRASS_DEVICE_PACK", None)
        env.update(extra)
        r = subprocess.run([cli, "--dump-handoff", "--timestamp", "17_10_2026_120000", "-o", "out", path], capture_output=True, timeout=600,
                           env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()
        assert (b"packed on the device" in r.stderr) == bool(extra), r.stderr.decode()
        outs[tag] = (r.stdout, {p.name: p.read_bytes() for p in sorted(d.iterdir())})
        shutil.rmtree(d)
    assert sorted(outs["host"][1]) == sorted(outs["device"][1])
    assert "crass.crispr" in outs["host"][1] and "crass_hip_handoff.tsv" in outs["host"][1]
    for name in outs["host"][1]:
        assert outs["host"][1][name] == outs["device"][1][name], name
