"""Read text fetched back out of the resident packed set (crass_hip_fetch_text, crass_hip_fetch_text_device,
crass_hip_fetch_record_text, crass_hip_group_fetch_text; k_fetch_text in pack.hip).  Every comparison is exact equality, and
the expected text is the INPUT text itself, or its reverse complement by the rule written out below — never anything the
library computed."""
import os

import numpy as np
import pytest

from tests import text_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
SETS = ["uniform150", "trimmed", "ragged", "odd_bytes", "exc_ends", "all_exc", "empty_reads", "n1", "n63", "n64", "n65", "long_ragged"]
INVALID_ARG, STATE, OVERFLOW = 1, 6, 8


def _comp_table():
    """reverseComplement's table: the pairs ACBDKRSWN <-> TGVHMYSWN in both cases, U -> A, u -> a, entry 96 -> 64, everything
    else itself; a byte b is looked up at b & 127"""
    t = list(range(128))
    for a, b in zip("ACBDKRSWN", "TGVHMYSWN"):
        for x, y in ((a, b), (b, a), (a.lower(), b.lower()), (b.lower(), a.lower())):
            t[ord(x)] = ord(y)
    t[ord("U")], t[ord("u")], t[96] = ord("A"), ord("a"), 64
    return bytes(t[b & 127] for b in range(256))


COMP = _comp_table()


def revcomp(s):
    return s.translate(COMP)[::-1]


def test_the_rule_itself():
    assert revcomp(b"ACGTN") == b"NACGT" and revcomp(b"acgu") == b"acgt" and revcomp(b"AAC") == b"GTT"
    assert revcomp(b"\x00\xff`U") == b"A@\x7f\x00" and revcomp(b"") == b""


@pytest.fixture(scope="module")
def ca():
    import crass_amd
    from crass_amd import build
    build.build()
    crass_amd.load()
    return crass_amd


class TextSet:
    def __init__(self, ca, name):
        self.name = name
        self.fwd = text_sets.make(ca, name)
        self.rc = [revcomp(s) for s in self.fwd]
        self.buf, self.off = text_sets.concat(self.fwd)
        n = self.n = len(self.fwd)
        self.exc = [i for i, s in enumerate(self.fwd) if set(s) - set(b"ACGT")]
        rng = np.random.default_rng(sum(name.encode()))
        lists = [("in order", np.arange(n)), ("reversed", np.arange(n)[::-1]), ("random", rng.integers(0, n, 500)),
                 ("first", np.array([0])), ("last", np.array([n - 1])), ("none", np.zeros(0, np.int64))]
        if self.exc:
            lists.append(("an exception read", np.array([self.exc[len(self.exc) // 2]])))
        assert len(np.unique(lists[2][1])) < 500 or n > 5000        # the random list repeats reads
        self.lists = []
        for lname, idx in lists:
            idx = np.ascontiguousarray(idx, dtype=np.uint64)
            for fname, fl in (("forward", None), ("all reversed", np.ones(len(idx), np.uint8)),
                              ("mixed", rng.integers(0, 2, len(idx)).astype(np.uint8))):
                self.lists.append((lname + ", " + fname, idx, fl))

    def want(self, idx, flags):
        recs = [(self.rc if (flags is not None and flags[k]) else self.fwd)[int(i)] for k, i in enumerate(idx)]
        off = np.zeros(len(recs) + 1, np.uint64)
        if recs:
            off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
        return b"".join(recs), off


_sets = {}


def get_set(ca, name):
    if name not in _sets:
        _sets[name] = TextSet(ca, name)
    return _sets[name]


def assert_text(res, chars, off, what):
    assert res.n == len(off) - 1, what
    assert res.off.dtype == np.uint64 and np.array_equal(res.off, off), what
    got = res.chars.tobytes()
    if got != chars:
        bad = next(i for i in range(min(len(got), len(chars))) if got[i] != chars[i]) if len(got) == len(chars) else -1
        k = int(np.searchsorted(off, bad, side="right")) - 1 if bad >= 0 else -1
        raise AssertionError("%s: text differs (lengths %d / %d), first at byte %d = record %d, byte %d of it: got %r, want %r"
                             % (what, len(got), len(chars), bad, k, bad - int(off[k]) if k >= 0 else -1, got[bad:bad + 20], chars[bad:bad + 20]))


def check_all_lists(eng, S, what, base=0):
    for lname, idx, flags in S.lists:
        chars, off = S.want(idx, flags)
        res = eng.fetch_text(idx + np.uint64(base), flags)
        assert_text(res, chars, off, "%s, %s" % (what, lname))
        if len(idx):
            k = len(idx) // 2
            assert res[k] == chars[int(off[k]):int(off[k + 1])] and res[-1] == chars[int(off[-2]):]


# ---- 1. every way a set becomes resident, every set, every layout ----
@pytest.mark.parametrize("name", SETS)
def test_text_comes_back_from_every_route(ca, name):
    import torch
    S = get_set(ca, name)
    with ca.SearchEngine() as eng:
        for pad in (0, 1, 2):
            what = "%s pad %d" % (name, pad)
            eng.load_text((S.buf, S.off), pad_uniform=pad)
            check_all_lists(eng, S, what + " load_text")
            t = torch.from_numpy(S.buf).to("cuda") if len(S.buf) else torch.zeros(0, dtype=torch.uint8, device="cuda")
            eng.attach_device_text(t, S.off, pad_uniform=pad)
            t.fill_(0x4E)                                # the context kept nothing of the text: overwrite it, then let it go
            torch.cuda.synchronize()
            del t
            torch.cuda.empty_cache()
            junk = torch.full((max(len(S.buf), 1),), 0x47, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            check_all_lists(eng, S, what + " attach_device_text")
            del junk
            pk = ca.PackedReads((S.buf, S.off), pad_uniform=pad)
            eng.load_reads(pk)
            check_all_lists(eng, S, what + " load_reads")
            pk.close()


def test_attached_packed_words(ca):
    """crass_hip_attach_device_reads: the caller's words (one stride, no exception reads, NO spare word behind the last read)"""
    import torch
    S = get_set(ca, "uniform150")
    pk = ca.PackedReads((S.buf, S.off), pad_uniform=1)
    words = torch.from_numpy(pk.packed_array().view(np.int32).copy()).to("cuda")
    assert words.numel() == S.n * 10
    torch.cuda.synchronize()
    with ca.SearchEngine() as eng:
        eng.attach_device_tensor(words, S.n, 150)
        check_all_lists(eng, S, "attach_device_reads")
    pk.close()


def test_global_indices_with_an_index_base(ca):
    S = get_set(ca, "trimmed")
    base = 5_000_000_000
    with ca.SearchEngine() as eng:
        eng.load_text((S.buf, S.off), pad_uniform=0, read_index_base=base)
        check_all_lists(eng, S, "load_text, index base", base=base)
        pk = ca.PackedReads((S.buf, S.off), pad_uniform=2)
        eng.load_reads(pk, read_index_base=base)
        check_all_lists(eng, S, "load_reads, index base", base=base)
        pk.close()
        for bad in (0, base - 1, base + S.n):
            with pytest.raises(ca.CrassError) as e:
                eng.fetch_text([base, bad])
            assert e.value.status == INVALID_ARG


# ---- 2. the device route ----
def test_device_route(ca):
    import torch
    S = get_set(ca, "ragged")
    lname, idx, flags = next(x for x in S.lists if x[0] == "random, mixed")
    chars, off = S.want(idx, flags)
    total = len(chars)
    want = np.frombuffer(chars, np.uint8)

    def filled(n):                                       # (the fill runs on torch's stream, the fetch on the engine's)
        t = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return t

    with ca.SearchEngine() as eng:
        eng.load_text((S.buf, S.off), pad_uniform=0)
        eng.set_stage_timing(0)
        assert_text(eng.fetch_text(idx, flags), chars, off, "host route")
        assert eng.last_fetch_ms() == 0.0
        eng.set_stage_timing(1)
        out = filled(total)
        got_off = eng.fetch_text(idx, flags, out=out)
        assert eng.last_fetch_ms() > 0.0
        assert np.array_equal(got_off, off) and np.array_equal(out.cpu().numpy(), want)
        small = filled(total - 1)      # one byte short
        with pytest.raises(ca.CrassError) as e:
            eng.fetch_text(idx, flags, out=small)
        assert e.value.status == OVERFLOW and np.array_equal(e.value.offsets, off)
        torch.cuda.synchronize()
        assert bool((small == 0xEE).all())
        big = filled(total + 64)        # 64 spare bytes stay as they were
        assert np.array_equal(eng.fetch_text(idx, flags, out=big), off)
        b = big.cpu().numpy()
        assert np.array_equal(b[:total], want) and np.all(b[total:] == 0xEE)
        for lead in (1, 5, 15):                          # a buffer that starts at an odd address: nothing in front of it is touched
            whole = filled(total + 96)
            view = whole[lead:lead + total]
            assert view.data_ptr() % 16 == lead
            assert np.array_equal(eng.fetch_text(idx, flags, out=view), off)
            w = whole.cpu().numpy()
            assert np.all(w[:lead] == 0xEE) and np.array_equal(w[lead:lead + total], want) and np.all(w[lead + total:] == 0xEE), lead
        empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
        assert eng.fetch_text([], None, out=empty).tolist() == [0]
        with pytest.raises(ca.CrassError) as e:
            eng.fetch_text(idx[:3], None, out=empty)
        assert e.value.status == OVERFLOW and np.array_equal(e.value.offsets, S.want(idx[:3], None)[1])


# ---- 3. errors leave everything as it was ----
def same_arrays(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert b[k] is not None and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_errors(ca):
    S = get_set(ca, "trimmed")
    lname, idx, flags = next(x for x in S.lists if x[0] == "random, mixed")
    chars, off = S.want(idx, flags)
    base = 1000
    with ca.SearchEngine() as eng:
        for call in (lambda: eng.fetch_text([0]), lambda: eng.fetch_record_text(1), lambda: eng.fetch_record_text(2)):
            with pytest.raises(ca.CrassError) as e:
                call()
            assert e.value.status == STATE               # nothing resident yet
        eng.load_text((S.buf, S.off), pad_uniform=2, read_index_base=base)
        res = eng.packed()
        before = res.arrays()
        res.close()

        def intact(what):
            r = eng.packed()
            same_arrays(before, r.arrays())
            r.close()
            assert_text(eng.fetch_text(idx + np.uint64(base), flags), chars, off, what)

        intact("first fetch")
        cases = [(lambda: eng.fetch_text([base - 1]), INVALID_ARG), (lambda: eng.fetch_text([base + S.n]), INVALID_ARG),
                 (lambda: eng.fetch_text([base, base + 1, base + S.n, base + 2], [0, 1, 0, 1]), INVALID_ARG),
                 (lambda: eng.fetch_text([0]), INVALID_ARG),
                 (lambda: eng.fetch_record_text(0), INVALID_ARG), (lambda: eng.fetch_record_text(3), INVALID_ARG),
                 (lambda: eng.fetch_record_text(1), STATE), (lambda: eng.fetch_record_text(2), STATE)]
        for k, (call, status) in enumerate(cases):
            with pytest.raises(ca.CrassError) as e:
                call()
            assert e.value.status == status, k
            intact("after error case %d" % k)
        assert eng.lib.crass_hip_fetch_text(eng.h, None, None, 3, None) == INVALID_ARG
        from crass_amd import _abi
        import ctypes as C
        assert eng.lib.crass_hip_fetch_text(eng.h, None, None, 3, C.byref(_abi.Text())) == INVALID_ARG      # no index array
        eng.seed_scan()
        eng.fetch_record_text(1)
        eng.merge()
        with pytest.raises(ca.CrassError) as e:
            eng.fetch_record_text(2)                     # no recruit yet
        assert e.value.status == STATE
        intact("after fetch_record_text(2) without a recruit")


# ---- 4. RH_Seq of the records of a full step ----
@pytest.mark.parametrize("fname", sorted(os.listdir(DATA)))
def test_record_text_of_a_full_step(ca, fname):
    f = ca.FastxFile(os.path.join(DATA, fname))
    hid = None if f.unique_headers() else f.header_id
    with ca.SearchEngine() as eng:
        eng.load_text((f.seq, f.seq_off), pad_uniform=2, header_id=hid)
        cand = eng.seed_scan()
        eng.merge()
        rec = eng.recruit()
        for pass_, rs in ((1, cand), (2, rec)):
            t = eng.fetch_record_text(pass_)
            assert t.n == rs.n and len(t.off) == rs.n + 1, (fname, pass_)
            for k in range(rs.n):
                i = int(rs.read_idx[k])
                seq = f.seq[int(f.seq_off[i]):int(f.seq_off[i + 1])].tobytes()
                assert t[k] == (seq if rs.low_lexi[k] else revcomp(seq)), (fname, pass_, k, i)


# ---- 5. a group: indices routed to the shards ----
def test_group_routes_indices_to_their_shards(ca):
    S = get_set(ca, "ragged")
    rng = np.random.default_rng(5)
    idx = np.concatenate([rng.permutation(S.n), rng.integers(0, S.n, 300)]).astype(np.uint64)
    half = S.n // 2
    assert np.any((idx[:-1] < half) & (idx[1:] >= half)) and np.any((idx[:-1] >= half) & (idx[1:] < half))
    base = 77
    for flags in (None, rng.integers(0, 2, len(idx)).astype(np.uint8)):
        chars, off = S.want(idx, flags)
        pk = ca.PackedReads((S.buf, S.off), pad_uniform=0)
        with ca.SearchGroup([0, 0], local_copies=True) as g, ca.SearchEngine() as eng:
            with pytest.raises(ca.CrassError) as e:
                g.fetch_text([0])
            assert e.value.status == STATE
            g.load_reads(pk, read_index_base=base)
            eng.load_reads(pk, read_index_base=base)
            a = g.fetch_text(idx + np.uint64(base), flags)
            b = eng.fetch_text(idx + np.uint64(base), flags)
            assert_text(b, chars, off, "one context")
            assert_text(a, chars, off, "group of two")
            assert np.array_equal(a.off, b.off) and np.array_equal(a.chars, b.chars)
            assert g.fetch_text([], None).n == 0
            with pytest.raises(ca.CrassError) as e:
                g.fetch_text([base + S.n])
            assert e.value.status == INVALID_ARG
        pk.close()


def test_group_of_one_rank_over_rccl_beside_torch(ca):
    """a group on the RCCL collective proper (one rank), in a process that imported torch AFTER the library: the torch wheel
    brings its own RCCL and HIP runtime, and the group has to bind the RCCL of the runtime its streams belong to.  One step
    through the collective, then the records' text."""
    import torch  # noqa: F401
    S = get_set(ca, "uniform150")
    pk = ca.PackedReads((S.buf, S.off), pad_uniform=2)
    with ca.SearchGroup([0]) as g:
        assert g.rccl_ranks == 1
        g.load_reads(pk)
        g.step()
        lname, idx, flags = next(x for x in S.lists if x[0] == "random, mixed")
        chars, off = S.want(idx, flags)
        assert_text(g.fetch_text(idx, flags), chars, off, "group of one over RCCL")
    pk.close()
