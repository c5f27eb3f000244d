"""The found-name exchange's calls with everything in device memory, each against what it replaces, element for element:
names_of_device (k_nm_measure_idx, the three-launch prefix sum, k_nm_copy) against the host's crass_fastx_names_of;
names_find_device (k_hid_find_dev, k_hid_find_long) against crass_fastx_find_names; found_names_device against the names cut from
the header lines of the candidates; recruit(extra_found_device=...) (k_mark_found_skip) against recruit(extra_found=...)."""
import os
import random

import numpy as np
import pytest

from tests import fastx_sets, name_sets
from tests import recruit_sets as rs

pytestmark = pytest.mark.gpu

TEXTS = name_sets.texts()
NF = name_sets.NOT_FOUND
FILL = 0xA5
INVALID_ARG, STATE, OVERFLOW = 1, 6, 8


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
def T(ca):
    t = int(ca.load().crass_hip_names_scan_tile())
    assert t >= 64 and t % 64 == 0
    return t


def dev_bytes(data, lead=0, tail=64):
    """bytes in a device tensor that starts `lead` bytes behind an allocation, name bytes all around them"""
    import torch
    big = torch.full((len(data) + lead + tail,), 0x51, dtype=torch.uint8, device="cuda")
    t = big[lead:lead + len(data)]
    if len(data):
        t.copy_(torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()))
    return big, t


def dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def out_buffers(cap, lead, n):
    """an output of cap bytes `lead` bytes into an allocation filled with FILL, and n + 1 offsets"""
    import torch
    big = torch.full((cap + lead + 16,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    return big, (int(big.data_ptr()) + lead, cap), off


def names_of_check(ca, e, data, rp, idx, base, lead, cap=None, what=None):
    """names_of_device against names_of for one list and one capacity; the bytes around the output keep their fill"""
    ix = np.asarray(idx, np.uint64) + np.uint64(base)
    want_c, want_o = ca.names_of(data, rp, ix, idx_base=base)
    total = int(want_o[-1])
    cap = total if cap is None else cap
    big, out, off = out_buffers(cap, lead, len(ix))
    d_idx = dev_u64(ix)
    if cap < total:
        with pytest.raises(ca.CrassError) as err:
            e.names_of_device(d_idx, out, off, idx_base=base)
        assert err.value.status == OVERFLOW and err.value.total == total, what
    else:
        assert e.names_of_device(d_idx, out, off, idx_base=base) == total, what
    assert np.array_equal(host_u64(off), want_o), what
    got = big.cpu().numpy()
    m = min(cap, total)
    assert np.array_equal(got[lead:lead + m], want_c[:m]), what
    assert np.all(got[:lead] == FILL) and np.all(got[lead + m:] == FILL), what


def picks(name, n_reads):
    rng = random.Random("names_of_device:" + name)
    idx = list(range(n_reads)) + [rng.randrange(n_reads) for _ in range(n_reads + 5)]
    rng.shuffle(idx)
    return idx


# ---- 1. names out ----
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_names_of_device_equals_the_host_function(ca, eng, name):
    """every designed text (names of 0 .. 1000 bytes, CRLF, a last header without a line end), the file bytes and the output at
    every byte offset 0 .. 3, both index bases, and the capacity one short, exact and one long"""
    data, rp = TEXTS[name]
    idx = picks(name, len(rp) - 1)
    for lead in range(4):
        big, t = dev_bytes(data, lead)
        eng.names_build(t, rp)
        for olead in range(4):
            names_of_check(ca, eng, data, rp, idx, 7 * ((lead + olead) % 2), olead, what=(name, lead, olead))
    total = int(ca.names_of(data, rp, idx)[1][-1])
    for cap in (total - 1, total, total + 1):
        if cap >= 0:
            names_of_check(ca, eng, data, rp, idx, 0, 1, cap, what=(name, "cap", cap))
    eng.names_drop()


def test_names_of_device_counts_around_the_scan_tile(ca, eng, T):
    """n of 0, 1, around a wave and around one and two tiles of the prefix sum; records of empty names at the tile edges"""
    data, rp = TEXTS["lengths_fa"]
    n_reads = len(rp) - 1
    empty = [r for r in range(n_reads) if not name_sets.name_at(data, int(rp[r]))]
    assert empty
    big, t = dev_bytes(data, 3)
    eng.names_build(t, rp)
    rng = random.Random(11)
    for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        idx = [rng.randrange(n_reads) for _ in range(n)]
        for edge in (0, T - 1, T, 2 * T - 1, 2 * T, n - 1):
            if 0 <= edge < n:
                idx[edge] = empty[edge % len(empty)]
        names_of_check(ca, eng, data, rp, idx, 7, n % 4, what=("n", n))
        if n > 64:                                       # ... and the other way round: only the edges carry bytes
            idx2 = [empty[0]] * n
            for edge in (0, T - 1, T, 2 * T - 1, 2 * T, n - 1):
                if 0 <= edge < n:
                    idx2[edge] = idx[(edge + 1) % n]
            names_of_check(ca, eng, data, rp, idx2, 0, 2, what=("n edges", n))
    eng.names_drop()


def test_names_of_device_counts_beyond_one_step_of_the_top_scan(ca, eng, T):
    """256 T, 256 T + 1 and 2 * 256 T + 1 entries: the one block over the tile sums takes 256 tiles a step, so these lists take
    its second and third step, with the carry of the steps before in front.  Records of empty names at the entries 256 T - 1,
    256 T and the last; then the other way round, only those three carry bytes.  (Nearly all entries are records of names up to 8
    bytes, one in a thousand is any record: the output stays a few MB.)"""
    data, rp = TEXTS["lengths_fa"]
    n_reads = len(rp) - 1
    lens = np.asarray([len(name_sets.name_at(data, int(rp[r]))) for r in range(n_reads)])
    empty, short, named = np.flatnonzero(lens == 0), np.flatnonzero((lens > 0) & (lens <= 8)), np.flatnonzero(lens > 0)
    assert len(empty) and len(short) > 8 and lens.max() >= 1000
    S = 256 * T
    big, t = dev_bytes(data, 2)
    eng.names_build(t, rp)
    rng = np.random.default_rng(12)
    for n in (S, S + 1, 2 * S + 1):
        edges = [e for e in (S - 1, S, n - 1) if e < n]
        idx = short[rng.integers(0, len(short), n)]
        any_at = rng.integers(0, n, n // 1000)
        idx[any_at] = named[rng.integers(0, len(named), len(any_at))]
        idx[edges] = empty[:1]
        names_of_check(ca, eng, data, rp, idx, 7, n % 4, what=("n", n))
        idx2 = np.full(n, empty[0])
        idx2[edges] = named[rng.integers(0, len(named), len(edges))]
        names_of_check(ca, eng, data, rp, idx2, 0, 2, what=("n edges", n))
    eng.names_drop()


def test_names_of_device_errors(ca, T):
    lib = ca.load()
    data, rp = TEXTS["prefixes"]
    n_reads = len(rp) - 1
    big, t = dev_bytes(data)
    with ca.SearchEngine() as e:
        _, out, off = out_buffers(64, 0, 2)
        with pytest.raises(ca.CrassError) as err:
            e.names_of_device(dev_u64([0, 1]), out, off)
        assert err.value.status == STATE                  # no table
        e.names_build(t, rp)
        for idx, base in (([0, n_reads], 0), ([7, 3], 7), ([2 ** 64 - 1], 0), ([7] * (T + 3) + [n_reads + 7], 7)):
            obig, out, off = out_buffers(4096, 0, len(idx))
            with pytest.raises(ca.CrassError) as err:
                e.names_of_device(dev_u64(idx), out, off, idx_base=base)
            assert err.value.status == INVALID_ARG, (idx[-3:], base)
            assert np.all(obig.cpu().numpy() == FILL)    # no byte is written
        assert lib.crass_hip_fastx_names_of_device(e.h, None, 1, 0, None, 0, int(off.data_ptr()), None) == INVALID_ARG
        assert lib.crass_hip_fastx_names_of_device(e.h, int(off.data_ptr()), 1, 0, None, 0, None, None) == INVALID_ARG
        assert lib.crass_hip_fastx_names_of_device(e.h, int(off.data_ptr()), 1, 0, None, 5, int(off.data_ptr()), None) == INVALID_ARG


# ---- 2. names looked up ----
_want = {}


def want_of(ca, key, data, rp, q):
    if key not in _want:
        w = ca.find_names(data, rp, q)
        assert np.array_equal(w, name_sets.expected(data, rp, q)), key
        _want[key] = w
    return _want[key]


def find_check(ca, e, key, data, rp, lead=0, qlead=0, q=None, build=True):
    import torch
    q = name_sets.queries(data, rp) if q is None else q
    want = want_of(ca, key, data, rp, q)
    if build:
        big, t = dev_bytes(data, lead)
        e.names_build(t, rp)
    chars, off = name_sets.concat(q)
    qbig, qt = dev_bytes(chars.tobytes(), qlead, tail=8)
    assert qt.data_ptr() % 4 == qlead % 4 or not len(chars)
    out = torch.full((len(q) + 2,), 12345, dtype=torch.int64, device="cuda")
    e.names_find_device((int(qt.data_ptr()) if len(chars) else 0, len(chars)), dev_u64(off), (int(out.data_ptr()), len(q)))
    got = host_u64(out)
    assert np.array_equal(got[:len(q)], want), (key, lead, qlead, np.flatnonzero(got[:len(q)] != want)[:5])
    assert np.all(got[len(q):] == 12345)
    return want


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_names_find_device_equals_the_host_function(ca, eng, name):
    data, rp = TEXTS[name]
    for lead in range(4):
        find_check(ca, eng, name, data, rp, lead, (lead + 1) % 4)
    for qlead in (0, 2, 3):
        find_check(ca, eng, name, data, rp, 0, qlead, build=False)
    eng.names_drop()


@pytest.fixture(scope="module")
def many():
    rng = random.Random(5)
    recs = [fastx_sets.fq(b"lane%d:%d/1 c" % (i % 7, i // 3), fastx_sets.acgt(rng, 30)) for i in range(1500)]
    longs = [name_sets.rand_name(rng, rng.choice((260, 261, 300, 1000))) for _ in range(40)]
    recs += [fastx_sets.fa(nm, fastx_sets.acgt(rng, 20)) for nm in longs]
    data, rp = name_sets.build(recs)
    present = list(name_sets.first_by_name(data, rp))
    q = [rng.choice(present) if rng.random() < 0.6 else rng.choice(present) + rng.choice([b"0", b"/", b""]) for _ in range(700)]
    return data, rp, q, longs


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_query_counts(ca, eng, many, n):
    data, rp, q, longs = many
    find_check(ca, eng, "many %d" % n, data, rp, 2, 1, q[:n])
    eng.names_drop()


def test_long_queries_from_several_waves(ca, eng, many):
    """more than 64 queries of 260 bytes or more, spread over the waves of several blocks between short ones: each wave appends
    its own with one add, the wave kernel answers all of them"""
    data, rp, q, longs = many
    rng = random.Random(8)
    qq = list(q)
    for k in range(0, len(qq), 5):                       # 140 long queries: present, one byte off, one byte short
        nm = longs[(k // 5) % len(longs)]
        qq[k] = (nm, nm[:-1] + name_sets.other(nm[-1:]), nm[:-1] if len(nm) > 260 else nm + b"x")[(k // 5) % 3]
    qq[64:128] = [longs[i % len(longs)] for i in range(64)]      # a whole wave of them
    assert sum(len(x) >= 260 for x in qq) > 64
    want = find_check(ca, eng, "several waves", data, rp, 1, 3, qq)
    assert np.count_nonzero(want[64:128] != NF) == 64
    eng.names_drop()


def engine_with_hash_bits(ca, bits):
    old = os.environ.pop("CRASS_HID_TEST_HASH_BITS", None)
    if bits is not None:
        os.environ["CRASS_HID_TEST_HASH_BITS"] = str(bits)
    try:
        return ca.SearchEngine()                          # (the switch is read when the context is created)
    finally:
        os.environ.pop("CRASS_HID_TEST_HASH_BITS", None)
        if old is not None:
            os.environ["CRASS_HID_TEST_HASH_BITS"] = old


@pytest.mark.parametrize("bits", [None, 4, 0])
def test_probe_chains(ca, bits):
    data, rp = name_sets.chain(200)
    with engine_with_hash_bits(ca, bits) as e:
        find_check(ca, e, "chain 200", data, rp, 1, 2)
        d2, r2 = TEXTS["long_prefixes"]
        find_check(ca, e, "long_prefixes", d2, r2, 3, 1)


def test_names_find_device_errors(ca):
    import torch
    lib = ca.load()
    data, rp = TEXTS["repeats"]
    q = name_sets.queries(data, rp)
    want = ca.find_names(data, rp, q)
    chars, off = name_sets.concat(q)
    big, t = dev_bytes(data)
    qbig, qt = dev_bytes(chars.tobytes(), 1, tail=8)
    names = (int(qt.data_ptr()), len(chars))

    def run(e, offsets, n_name_bytes=None):
        out = torch.full((len(q),), 12345, dtype=torch.int64, device="cuda")
        e.names_find_device(names, dev_u64(offsets), out, n_name_bytes=n_name_bytes)
        return host_u64(out)

    with ca.SearchEngine() as e:
        with pytest.raises(ca.CrassError) as err:
            run(e, off)
        assert err.value.status == STATE                  # no table
        e.names_build(t, rp)
        assert np.array_equal(run(e, off), want)
        down = off.copy()
        down[3] = down[4] + 1                             # a decreasing pair: queries 2 and 3 are touched by it
        out = torch.full((len(q),), 12345, dtype=torch.int64, device="cuda")
        with pytest.raises(ca.CrassError) as err:
            e.names_find_device(names, dev_u64(down), out)
        assert err.value.status == INVALID_ARG
        got = host_u64(out)
        assert got[3] == NF                               # the bad query reads nothing and is not found
        keep = np.ones(len(q), bool)
        keep[2:4] = False
        assert np.array_equal(got[keep], want[keep])      # ... the others are answered
        with pytest.raises(ca.CrassError) as err:         # the last offset beyond the bytes the caller vouches for
            run(e, off, n_name_bytes=len(chars) - 1)
        assert err.value.status == INVALID_ARG
        beyond = off.copy()
        beyond[-1] += 1000
        with pytest.raises(ca.CrassError) as err:
            run(e, beyond)
        assert err.value.status == INVALID_ARG
        assert np.array_equal(run(e, off), want)          # the table answers as before
        o = dev_u64(off)
        assert lib.crass_hip_fastx_names_find_device(e.h, names[0], names[1], None, len(q), int(o.data_ptr())) == INVALID_ARG
        assert lib.crass_hip_fastx_names_find_device(e.h, names[0], names[1], int(o.data_ptr()), len(q), None) == INVALID_ARG
        assert lib.crass_hip_fastx_names_find_device(e.h, None, names[1], int(o.data_ptr()), len(q), int(o.data_ptr())) == INVALID_ARG
        assert lib.crass_hip_fastx_names_find_device(e.h, None, 0, None, 0, None) == 0
        # a table of no records: nothing is found
        e.names_build(t, np.asarray([len(data)], np.uint64))
        assert np.all(run(e, off) == NF)


# ---- 3. the round trip: pass 1's records -> their names, without their indices crossing to the host ----
def fq_of(recs):
    return b"".join(b"@" + nm + b" c" + nm + b"\n" + s + b"\n+\n" + bytes(70 + (k + i) % 40 for i in range(len(s))) + b"\n" for k, (nm, s) in enumerate(recs))


def synth_records(ca, n, L, per_million, seed):
    spec = ca.synth_spec(read_len=L, crispr_per_million=per_million, n_dr=8)
    asc = ca.unpack_ascii(ca.synth_packed(spec, 0, n), (L + 15) // 16, L, n)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = asc[i * L:(i + 1) * L].tobytes()
        if i % 11 == 0:
            s = s[:int(rng.integers(L // 2, L))]
        out.append((b"read%d/%d" % ((7 * i + 1) % n if i % 3 == 0 else i, 1 + i % 2) + (b"x" * 270 if i % 97 == 0 else b""), s))
    return out


@pytest.mark.parametrize("kind", ["dense_short", "long"])
def test_found_names_round_trip(ca, kind):
    import torch
    recs = synth_records(ca, 6000, 150, 60000, 3) if kind == "dense_short" else synth_records(ca, 240, 2100, 200000, 4)
    files = [fq_of(recs[:len(recs) // 2]), fq_of(recs[len(recs) // 2:])]
    with ca.SearchEngine() as e:
        lay = e.load_fastx_files(files)
        assert lay.n_reads == len(recs) and lay.max_len == (150 if kind == "dense_short" else 2100)
        e.names_build(None, None)
        cand = e.seed_scan()
        e.merge()
        idx = np.asarray(cand.read_idx, np.uint64)
        assert len(idx) > (100 if kind == "dense_short" else 10)
        addr, nb = e.resident_fastx()
        chars, off, name_len = e.fetch_header_lines(addr, np.append(lay.rec_pos[:-1], nb), idx)
        names = [bytes(chars[int(off[k]):int(off[k]) + int(name_len[k])]) for k in range(len(idx))]
        assert names == [recs[int(r)][0] for r in idx]
        want_c, want_o = name_sets.concat(names)
        total = int(want_o[-1])
        big, out, d_off = out_buffers(total, 3, len(idx))
        assert e.found_names_device(out, d_off) == (len(idx), total)
        assert np.array_equal(host_u64(d_off), want_o)
        got = big.cpu().numpy()
        assert np.array_equal(got[3:3 + total], want_c) and np.all(got[3 + total:] == FILL)
        # too few bytes, too few offsets: the counts come back, nothing is written behind the capacity
        big, out, d_off = out_buffers(total - 1, 0, len(idx))
        with pytest.raises(ca.CrassError) as err:
            e.found_names_device(out, d_off)
        assert err.value.status == OVERFLOW and (err.value.n, err.value.total) == (len(idx), total)
        got = big.cpu().numpy()
        assert np.array_equal(host_u64(d_off), want_o) and np.array_equal(got[:total - 1], want_c[:total - 1]) and np.all(got[total - 1:] == FILL)
        big, out, _ = out_buffers(total, 0, 0)
        short = torch.full((len(idx),), -1, dtype=torch.int64, device="cuda")      # room for len(idx) - 1 names
        with pytest.raises(ca.CrassError) as err:
            e.found_names_device(out, short)
        assert err.value.status == OVERFLOW and (err.value.n, err.value.total) == (len(idx), total)
        assert np.all(big.cpu().numpy() == FILL) and np.all(short.cpu().numpy() == -1)
        e.names_drop()
        with pytest.raises(ca.CrassError) as err:
            e.found_names_device(out, d_off)
        assert err.value.status == STATE


# ---- 4. names marked: pass 2 with a device list that may hold "not found" ----
def fields(r):
    return (r.read_idx.tolist(), r.low_lexi.tolist(), r.start.tolist(), r.end.tolist(), r.dr_len.tolist(), r.token.tolist(),
            [r.dr(k) for k in range(len(r.read_idx))])


def test_recruit_with_a_device_list(ca):
    c = rs.case("mode0", "u150", 2003)
    want = sorted(c.want())
    n = len(c.seqs)
    hid = np.arange(n, dtype=np.uint64)
    for a, b in zip(want[0::4], want[1::4]):             # every fourth recruitable read shares its header with the next one
        hid[b] = a
    rng = random.Random(2)
    a = []
    for r in want[0::3]:                                 # a third of the recruitable reads, "not found" entries between them
        a += [r] + [NF] * rng.randrange(3)
    a = np.asarray([NF] + a + [want[0]], np.uint64)      # ... in front, and a repeat
    listed = a[a != NF]
    packed = ca.PackedReads(c.seqs, 0)

    def run(extra=None, dev=None):
        with ca.SearchEngine() as e:
            e.load_reads(packed, hid)
            e.set_patterns(c.patterns)
            got = e.recruit(extra, extra_found_device=None if dev is None else dev_u64(dev))
            return fields(got)

    try:
        plain = run()
        host = run(extra=listed)
        ref = rs.find_singletons(c.seqs, c.patterns, [int(x) for x in listed], hid)
        assert host[0] == [r[0] for r in ref] and len(host[0]) < len(plain[0]) - len(set(listed.tolist()))
        assert run(dev=a) == host                         # field by field
        assert run(dev=np.full(5, NF, np.uint64)) == plain
        assert run(dev=np.zeros(0, np.uint64)) == plain
        # host and device lists together: their union
        host_part, dev_part = listed[:len(listed) // 2], a[len(a) // 2:]
        union = np.union1d(host_part, dev_part[dev_part != NF])
        assert len(union) > max(len(host_part), np.count_nonzero(dev_part != NF))
        assert run(extra=host_part, dev=dev_part) == run(extra=union)
        # an entry equal to n_reads: an invalid argument, and no pass-2 result is left
        with ca.SearchEngine() as e:
            e.load_reads(packed, hid)
            e.set_patterns(c.patterns)
            e.recruit()
            bad = a.copy()
            bad[len(bad) // 2] = n
            with pytest.raises(ca.CrassError) as err:
                e.recruit(extra_found_device=dev_u64(bad))
            assert err.value.status == INVALID_ARG
            with pytest.raises(ca.CrassError) as err:
                e.recruits()
            assert err.value.status == STATE
            assert fields(e.recruit()) == plain           # nothing of the refused list was marked
    finally:
        packed.close()
