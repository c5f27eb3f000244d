"""Python host layer over the C ABI (include/crass_hip.h).

Used by the tests, bench.py and the multi-GPU driver (torch.distributed is plumbing only).
The compiled C++ adapter with the reference's own function shapes (searchFile /
createNonRedundantSet / findSingletons / addReadHolder) lives in csrc/adapter/ — see
INTEGRATION.md.  Nothing here computes search results on the CPU.
"""
import ctypes as C

import numpy as np

from . import _abi


class CrassError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        msg = _abi.load().crass_hip_strerror(status).decode()
        super().__init__("%s: %s (status %d)" % (where or "crass_hip", msg, status))


def _chk(status, where):
    if status != 0:
        raise CrassError(status, where)


def default_params(**kw):
    p = _abi.Params()
    _abi.load().crass_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _np(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).view(dtype).copy()


def _npv(addr, n, dtype):
    """n elements of dtype at the raw address addr (a c_void_p field) as a numpy copy"""
    if n == 0 or not addr:
        return np.zeros(0, dtype)
    ct = {np.uint8: C.c_uint8, np.uint32: C.c_uint32, np.uint64: C.c_uint64}[dtype]
    return np.ctypeslib.as_array(C.cast(C.c_void_p(addr), C.POINTER(ct)), shape=(int(n),)).view(dtype).copy()


def concat(items):
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        off[1:] = np.cumsum([len(s) for s in items], dtype=np.uint64)
    buf = np.frombuffer(b"".join(items), dtype=np.uint8).copy() if items else np.zeros(0, np.uint8)
    return buf, off


class PackedReads:
    """2-bit packed reads + exception list produced by the C++ packer (crass_pack_reads)."""

    def __init__(self, seqs, pad_uniform=False):
        lib = _abi.load()
        if isinstance(seqs, (list, tuple)) and (not seqs or isinstance(seqs[0], (bytes, bytearray))):
            buf, off = concat(list(seqs))
        else:
            buf, off = seqs
        self._src = (buf, off)
        self.p = _abi.Packed()
        _chk(lib.crass_pack_reads(buf.ctypes.data, off.ctypes.data, len(off) - 1, int(pad_uniform), C.byref(self.p)),
             "crass_pack_reads")
        self.header_id = None

    @property
    def reads(self):
        return self.p.reads

    @property
    def n_reads(self):
        return int(self.p.reads.n_reads)

    def packed_array(self):
        r = self.p.reads
        if r.stride_words:
            n = int(r.n_reads) * int(r.stride_words)
        else:
            raise ValueError("ragged layout")
        return np.ctypeslib.as_array(C.cast(r.packed, _abi.u32p), shape=(n,))

    def close(self):
        if self.p.owner:
            _abi.load().crass_free_packed(C.byref(self.p))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def packed_arrays(r):
    """Every array of a crass_reads with HOST pointers (_abi.Reads) as numpy copies, by field name; arrays the set does not
    have are None.  `packed` includes padding and the four tail words."""
    n, ne = int(r.n_reads), int(r.n_exceptions)
    stride, ulen = int(r.stride_words), int(r.uniform_len)
    d = {"n_reads": n, "stride_words": stride, "uniform_len": ulen, "n_exceptions": ne, "read_index_base": int(r.read_index_base)}
    d["word_off"] = None if stride else _npv(r.word_off, n + 1, np.uint64)
    d["lengths"] = None if ulen else _npv(r.lengths, n, np.uint32)
    total = n * stride if stride else (int(d["word_off"][n]) if n else 0)
    d["packed"] = _npv(r.packed, total + 4, np.uint32)
    d["exc_read"] = _npv(r.exc_read, ne, np.uint64)
    d["exc_off"] = _npv(r.exc_off, ne + 1, np.uint64)
    d["exc_bytes"] = _npv(r.exc_bytes, int(d["exc_off"][ne]) if ne else 0, np.uint8)
    d["header_id"] = _npv(r.header_id, n, np.uint64) if r.header_id else None
    return d


class ResidentReads:
    """A context's resident read set copied back to the host (crass_hip_get_packed); usable wherever a PackedReads is."""

    def __init__(self, engine):
        self.p = _abi.Packed()
        _chk(engine.lib.crass_hip_get_packed(engine.h, C.byref(self.p)), "crass_hip_get_packed")
        self.header_id = None

    @property
    def reads(self):
        return self.p.reads

    @property
    def n_reads(self):
        return int(self.p.reads.n_reads)

    def arrays(self):
        return packed_arrays(self.p.reads)

    def close(self):
        if self.p.owner:
            _abi.load().crass_free_packed(C.byref(self.p))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Text:
    """Records of sequence text (crass_text): `chars` (uint8) and `off` (uint64, n + 1) are numpy VIEWS of the memory the
    library owns — valid until the owner's next fetch, load or close; t[k] copies record k out as bytes."""

    def __init__(self, v):
        self.n = int(v.n)
        self.off = np.ctypeslib.as_array(v.off, shape=(self.n + 1,))
        total = int(self.off[self.n])
        self.chars = np.ctypeslib.as_array(v.chars, shape=(total,)) if total else np.zeros(0, np.uint8)

    def __len__(self):
        return self.n

    def __getitem__(self, k):
        k = int(k)
        if k < 0:
            k += self.n
        if not 0 <= k < self.n:
            raise IndexError(k)
        return self.chars[int(self.off[k]):int(self.off[k + 1])].tobytes()


def _fetch_args(idx, revcomp):
    a = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
    rc = None
    if revcomp is not None:
        rc = np.ascontiguousarray(np.asarray(revcomp).reshape(-1) != 0, dtype=np.uint8)
        if len(rc) != len(a):
            raise ValueError("one reverse-complement flag per index")
    return a, rc


def pack_layout(offsets, pad_uniform):
    """(stride_words, uniform_len) the packers give reads with these byte offsets (crass_pack_layout; no GPU needed)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    st, ul = C.c_uint32(), C.c_uint32()
    _chk(_abi.load().crass_pack_layout(off.ctypes.data, len(off) - 1, int(pad_uniform), C.byref(st), C.byref(ul)), "crass_pack_layout")
    return int(st.value), int(ul.value)


def pack_code4(four_bytes):
    """(codes, bad bits) of four sequence bytes given as a little-endian uint32 (crass_pack_code4; no GPU needed)."""
    bad = C.c_uint32()
    code = _abi.load().crass_pack_code4(int(four_bytes) & 0xFFFFFFFF, C.byref(bad))
    return int(code), int(bad.value)


class FastxLayout:
    """What the record scan found in the raw bytes of a FASTA / FASTQ file (crass_fastx_layout), as numpy copies: n_reads, format
    (b">" or b"@"; b"" when unknown), max_len, rec_pos / seq_off (uint64, n_reads + 1); a declined input has accepted False,
    decline_reason / decline_pos and empty arrays."""

    def __init__(self, v):
        self.n_reads = int(v.n_reads)
        self.format = bytes([v.format]) if v.format else b""
        self.decline_reason, self.decline_pos = int(v.decline_reason), int(v.decline_pos)
        self.accepted = self.decline_reason == 0
        self.max_len = int(v.max_len)
        have = bool(v.rec_pos) and bool(v.seq_off)
        self.rec_pos = _np(v.rec_pos, self.n_reads + 1, np.uint64) if have else np.zeros(0, np.uint64)
        self.seq_off = _np(v.seq_off, self.n_reads + 1, np.uint64) if have else np.zeros(0, np.uint64)


class FastxDeclined(CrassError):
    """The record scan declined the input (status 2): `layout` says why and where; the caller takes the host readers."""

    def __init__(self, status, where, layout):
        super().__init__(status, where)
        self.layout = layout


def _bytes_arg(buf):
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(buf), dtype=np.uint8)
    return np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)


def fastx_scan_host(buf, fastq_class=0):
    """The record scan of the raw bytes of a FASTA / FASTQ file on the host (crass_fastx_scan_host; no GPU needed): a
    FastxLayout, accepted or declined.  fastq_class 1: FASTQ by the wrapped rule (crass_fastx_scan_host_class)."""
    lib = _abi.load()
    a = _bytes_arg(buf)
    v = _abi.FastxLayoutC()
    if fastq_class:
        fn, st = "crass_fastx_scan_host_class", lib.crass_fastx_scan_host_class(a.ctypes.data if len(a) else None, len(a), int(fastq_class), C.byref(v))
    else:
        fn, st = "crass_fastx_scan_host", lib.crass_fastx_scan_host(a.ctypes.data if len(a) else None, len(a), C.byref(v))
    try:
        if st not in (0, 2):
            raise CrassError(st, fn)
        return FastxLayout(v)
    finally:
        lib.crass_fastx_layout_free(C.byref(v))


class BgzfDeclined(CrassError):
    """The BGZF index or a member's inflate declined the input (status 2): `reason` (inflate_core.h: 1 .. 9 a member's deflate data,
    10 not BGZF), `member` and `in_pos` (the file position of that member's first byte); the caller takes the host readers."""

    def __init__(self, status, where, verdict):
        super().__init__(status, where)
        self.reason, self.member, self.in_pos = int(verdict.reason), int(verdict.member), int(verdict.in_pos)
        self.verdict = (self.reason, self.member, self.in_pos)


class BgzfIndex:
    """Where the members of a BGZF file are (crass_bgzf_index): n_members, in_off / out_off (uint64, n_members + 1), data_off
    (uint64, n_members: where each member's deflate data starts), n_text = out_off[-1]."""

    def __init__(self, in_off, out_off, data_off):
        self.in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        self.out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
        self.data_off = np.ascontiguousarray(data_off, dtype=np.uint64)
        self.n_members = len(self.data_off)
        if len(self.in_off) != self.n_members + 1 or len(self.out_off) != self.n_members + 1:
            raise ValueError("a BGZF index has n + 1 input and output offsets for n members")
        self.n_text = int(self.out_off[-1])

    def _c(self):
        v = _abi.BgzfIndexC()
        v.n_members = self.n_members
        v.in_off = self.in_off.ctypes.data_as(_abi.u64p)
        v.out_off = self.out_off.ctypes.data_as(_abi.u64p)
        v.data_off = self.data_off.ctypes.data_as(_abi.u64p) if self.n_members else None
        return v


def bgzf_index(buf):
    """The walk over the members' headers and trailers of a BGZF file's bytes (crass_bgzf_index_host; no GPU needed): a BgzfIndex;
    raises BgzfDeclined (reason 10) for anything else, a plain .gz among it."""
    lib = _abi.load()
    a = _bytes_arg(buf)
    v = _abi.BgzfIndexC()
    st = lib.crass_bgzf_index_host(a.ctypes.data if len(a) else None, len(a), C.byref(v))
    try:
        if st == 2:
            raise BgzfDeclined(st, "crass_bgzf_index_host", v.decline)
        _chk(st, "crass_bgzf_index_host")
        n = int(v.n_members)
        return BgzfIndex(_np(v.in_off, n + 1, np.uint64).copy(), _np(v.out_off, n + 1, np.uint64).copy(), _np(v.data_off, n, np.uint64).copy())
    finally:
        lib.crass_bgzf_index_free(C.byref(v))


def bgzf_inflate_host(buf, index=None):
    """The text of a BGZF file's bytes, member after member through the decoder the kernel runs (crass_bgzf_inflate_host; no GPU
    needed): a uint8 array; raises BgzfDeclined with the verdict.  index: a BgzfIndex of the same bytes (default: bgzf_index(buf))."""
    lib = _abi.load()
    a = _bytes_arg(buf)
    ix = bgzf_index(a) if index is None else index
    out = np.zeros(ix.n_text, np.uint8)
    ver = _abi.BgzfVerdict()
    ixc = ix._c()
    st = lib.crass_bgzf_inflate_host(a.ctypes.data if len(a) else None, len(a), C.byref(ixc), out.ctypes.data if len(out) else None, len(out), C.byref(ver))
    if st == 2:
        raise BgzfDeclined(st, "crass_bgzf_inflate_host", ver)
    _chk(st, "crass_bgzf_inflate_host")
    return out


class GzipPlan:
    """What the gzip rule decided (crass_gzip_plan), as numpy copies: n_chunks, n_chain, start_bit (uint64, ~0: none), link (uint32:
    a chunk, or LINK_END / LINK_UNFINISHED / LINK_BAD / LINK_NONE) and text_len (uint64), one entry per chunk."""
    LINK_END, LINK_UNFINISHED, LINK_BAD, LINK_NONE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC

    def __init__(self, v):
        n = int(v.n_chunks)
        self.n_chunks, self.n_chain = n, int(v.n_chain)
        self.start_bit = _np(v.start_bit, n, np.uint64).copy() if n else np.zeros(0, np.uint64)
        self.link = _np(v.link, n, np.uint32).copy() if n else np.zeros(0, np.uint32)
        self.text_len = _np(v.text_len, n, np.uint64).copy() if n else np.zeros(0, np.uint64)


def gzip_inflate_host(buf, chunk_bytes=0, out_cap=None, with_plan=False):
    """The text of a plain (single-member) gzip file's bytes, chunk by chunk through the rule the kernels run
    (crass_gzip_inflate_host; no GPU needed): a uint8 array, with with_plan (text, GzipPlan).  chunk_bytes: 0 is the default.
    Raises BgzfDeclined with the verdict (its `plan` holds the GzipPlan when the header parsed); out_cap smaller than the text
    raises CrassError with status 8 and the text's size in its `n_text`."""
    lib = _abi.load()
    a = _bytes_arg(buf)
    ptr = a.ctypes.data if len(a) else None
    n_text, ver, pc = C.c_uint64(0), _abi.BgzfVerdict(), _abi.GzipPlanC()
    try:
        st = lib.crass_gzip_inflate_host(ptr, len(a), int(chunk_bytes), None, 0, C.byref(n_text), C.byref(pc), C.byref(ver))
        plan = GzipPlan(pc)
    finally:
        lib.crass_gzip_plan_free(C.byref(pc))
    if st == 2:
        e = BgzfDeclined(st, "crass_gzip_inflate_host", ver)
        e.plan = plan
        raise e
    if st not in (0, 8):
        _chk(st, "crass_gzip_inflate_host")
    cap = int(n_text.value) if out_cap is None else int(out_cap)
    out = np.zeros(cap, np.uint8)
    st = lib.crass_gzip_inflate_host(ptr, len(a), int(chunk_bytes), out.ctypes.data if cap else None, cap, C.byref(n_text), None, C.byref(ver))
    if st == 2:
        e = BgzfDeclined(st, "crass_gzip_inflate_host", ver)
        e.plan = plan
        raise e
    if st == 8:
        e = CrassError(st, "crass_gzip_inflate_host")
        e.n_text, e.out = int(n_text.value), out
        raise e
    _chk(st, "crass_gzip_inflate_host")
    out = out[:int(n_text.value)]
    return (out, plan) if with_plan else out


def _gzip_guess_cap(a):
    """room for the text a gzip trailer promises (ISIZE, the file's last 4 bytes)"""
    return int.from_bytes(a[-4:].tobytes(), "little") if len(a) >= 18 else 0


def _gzip_ranges_call(fn, call, a, out_cap, with_plan):
    """One call of a ranges inflate (call(out_ptr, cap, n_text, plan, verdict) -> status) with room for the text the trailer
    promises, a second one where the text is larger; results and errors as gzip_inflate_host."""
    lib = _abi.load()
    cap = _gzip_guess_cap(a) if out_cap is None else int(out_cap)
    while True:
        out = np.zeros(cap, np.uint8)
        n_text, ver, pc = C.c_uint64(0), _abi.BgzfVerdict(), _abi.GzipPlanC()
        try:
            st = call(out.ctypes.data if cap else None, cap, C.byref(n_text), C.byref(pc), C.byref(ver))
            plan = GzipPlan(pc)
        finally:
            lib.crass_gzip_plan_free(C.byref(pc))
        if st == 8 and out_cap is None:
            cap = int(n_text.value)
            continue
        break
    if st == 2:
        e = BgzfDeclined(st, fn, ver)
        e.plan = plan
        raise e
    if st == 8:
        e = CrassError(st, fn)
        e.n_text, e.out, e.plan = int(n_text.value), out, plan
        raise e
    _chk(st, fn)
    out = out[:int(n_text.value)]
    return (out, plan) if with_plan else out


def gzip_inflate_ranges_host(buf, n_ranges, chunk_bytes=0, nominal=None, out_cap=None, with_plan=False):
    """gzip_inflate_host by the rule a group's ranks run (crass_gzip_inflate_ranges_host; no GPU needed): the text cut into
    n_ranges ranges at nominal (n_ranges - 1 text positions; None: even), every range's elements decoded and their windows walked
    symbolically, the entry windows composed in order.  Results and errors as gzip_inflate_host, for every n_ranges."""
    lib = _abi.load()
    a = _bytes_arg(buf)
    nom = _nominal_arg(nominal, int(n_ranges))
    ptr = a.ctypes.data if len(a) else None
    return _gzip_ranges_call("crass_gzip_inflate_ranges_host", lambda o, cap, n, p, v: lib.crass_gzip_inflate_ranges_host(
        ptr, len(a), int(chunk_bytes), int(n_ranges), nom.ctypes.data if nom is not None and len(nom) else None, o, cap, n, p, v), a, out_cap, with_plan)


class GzipMembers:
    """The members of a plain gzip file (crass_gzip_members), as numpy copies: n_members, in_off (uint64 [n + 1]: the file byte of
    each member's header, in_off[n] the file's size) and text_off (uint64 [n + 1]: member m is text[text_off[m] : text_off[m + 1]])."""

    def __init__(self, v):
        n = int(v.n_members)
        self.n_members = n
        self.in_off = _np(v.in_off, n + 1, np.uint64).copy() if v.in_off else np.zeros(0, np.uint64)
        self.text_off = _np(v.text_off, n + 1, np.uint64).copy() if v.text_off else np.zeros(0, np.uint64)


def gzip_inflate_members_host(buf, chunk_bytes=0, out_cap=None, with_plan=False):
    """gzip_inflate_host for a plain gzip file of any number of members (crass_gzip_inflate_members_host): a uint8 array, with
    with_plan (text, GzipPlan, GzipMembers).  Raises as gzip_inflate_host does; for reasons 7 / 8 / 9 the verdict's `member` is the
    gzip member and `in_pos` the file byte of its header."""
    lib = _abi.load()
    a = _bytes_arg(buf)
    ptr = a.ctypes.data if len(a) else None
    fn = "crass_gzip_inflate_members_host"
    n_text, ver, pc, mc = C.c_uint64(0), _abi.BgzfVerdict(), _abi.GzipPlanC(), _abi.GzipMembersC()
    try:
        st = lib.crass_gzip_inflate_members_host(ptr, len(a), int(chunk_bytes), None, 0, C.byref(n_text), C.byref(pc), None, C.byref(ver))
        plan = GzipPlan(pc)
    finally:
        lib.crass_gzip_plan_free(C.byref(pc))
    if st == 2:
        e = BgzfDeclined(st, fn, ver)
        e.plan = plan
        raise e
    if st not in (0, 8):
        _chk(st, fn)
    cap = int(n_text.value) if out_cap is None else int(out_cap)
    out = np.zeros(cap, np.uint8)
    try:
        st = lib.crass_gzip_inflate_members_host(ptr, len(a), int(chunk_bytes), out.ctypes.data if cap else None, cap, C.byref(n_text), None,
                                                 C.byref(mc), C.byref(ver))
        members = GzipMembers(mc)
    finally:
        lib.crass_gzip_members_free(C.byref(mc))
    if st == 2:
        e = BgzfDeclined(st, fn, ver)
        e.plan = plan
        raise e
    if st == 8:
        e = CrassError(st, fn)
        e.n_text, e.out = int(n_text.value), out
        raise e
    _chk(st, fn)
    out = out[:int(n_text.value)]
    return (out, plan, members) if with_plan else out


def _gzip_members_ranges_call(fn, call, a, out_cap, with_plan):
    """_gzip_ranges_call for a members inflate (call(out_ptr, cap, n_text, plan, members, verdict) -> status): with with_plan
    (text, GzipPlan, GzipMembers)."""
    lib = _abi.load()
    cap = _gzip_guess_cap(a) if out_cap is None else int(out_cap)
    while True:
        out = np.zeros(cap, np.uint8)
        n_text, ver, pc, mc = C.c_uint64(0), _abi.BgzfVerdict(), _abi.GzipPlanC(), _abi.GzipMembersC()
        try:
            st = call(out.ctypes.data if cap else None, cap, C.byref(n_text), C.byref(pc), C.byref(mc), C.byref(ver))
            plan, members = GzipPlan(pc), GzipMembers(mc)
        finally:
            lib.crass_gzip_plan_free(C.byref(pc))
            lib.crass_gzip_members_free(C.byref(mc))
        if st == 8 and out_cap is None:
            cap = int(n_text.value)
            continue
        break
    if st == 2:
        e = BgzfDeclined(st, fn, ver)
        e.plan = plan
        raise e
    if st == 8:
        e = CrassError(st, fn)
        e.n_text, e.out, e.plan = int(n_text.value), out, plan
        raise e
    _chk(st, fn)
    out = out[:int(n_text.value)]
    return (out, plan, members) if with_plan else out


def gzip_inflate_members_ranges_host(buf, n_ranges, chunk_bytes=0, nominal=None, out_cap=None, with_plan=False):
    """gzip_inflate_members_host by the rule a group's ranks run (crass_gzip_inflate_members_ranges_host; no GPU needed): the text
    cut into n_ranges ranges at nominal (n_ranges - 1 text positions; None: even), every range's elements decoded with member-end
    records of its own, windows walked symbolically with dead entries as 0, the members' CRC-32 joined from pieces.  Results and
    errors as gzip_inflate_members_host, for every n_ranges; with with_plan (text, GzipPlan, GzipMembers)."""
    lib = _abi.load()
    a = _bytes_arg(buf)
    nom = _nominal_arg(nominal, int(n_ranges))
    ptr = a.ctypes.data if len(a) else None
    return _gzip_members_ranges_call("crass_gzip_inflate_members_ranges_host", lambda o, cap, n, p, m, v: lib.crass_gzip_inflate_members_ranges_host(
        ptr, len(a), int(chunk_bytes), int(n_ranges), nom.ctypes.data if nom is not None and len(nom) else None, o, cap, n, p, m, v), a, out_cap,
        with_plan)


class FastxFilesLayout:
    """Several files as one read set (crass_fastx_files_layout), as numpy copies: n_files, n_reads, max_len, file_read_base /
    file_byte_base (uint64, n_files + 1; byte bases and rec_pos are ARENA positions: every file's text with a "\\n" behind it),
    formats (a list of b">" / b"@"), rec_pos / seq_off (uint64, n_reads + 1).  A declined set has accepted False, decline_file,
    and either decline_reason / decline_pos (a FASTA / FASTQ decline, the position inside that file) or bgzf = (reason, member,
    in_pos) (a compression decline), and empty arrays."""

    def __init__(self, v):
        self.n_files, self.n_reads, self.max_len = int(v.n_files), int(v.n_reads), int(v.max_len)
        self.decline_file, self.decline_reason, self.decline_pos = int(v.decline_file), int(v.decline_reason), int(v.decline_pos)
        self.bgzf = (int(v.bgzf.reason), int(v.bgzf.member), int(v.bgzf.in_pos))
        self.accepted = self.decline_file < 0
        have = bool(v.rec_pos) and bool(v.seq_off) and bool(v.file_read_base) and bool(v.file_byte_base) and bool(v.format)
        z = np.zeros(0, np.uint64)
        self.file_read_base = _np(v.file_read_base, self.n_files + 1, np.uint64).copy() if have else z
        self.file_byte_base = _np(v.file_byte_base, self.n_files + 1, np.uint64).copy() if have else z
        self.formats = [bytes([int(v.format[f]) & 0xFF]) for f in range(self.n_files)] if have else []
        self.rec_pos = _np(v.rec_pos, self.n_reads + 1, np.uint64).copy() if have else z
        self.seq_off = _np(v.seq_off, self.n_reads + 1, np.uint64).copy() if have else z

    @property
    def verdict(self):
        """what a declined set is compared by: (file, FASTA / FASTQ reason, position, BGZF verdict)"""
        return (self.decline_file, self.decline_reason, self.decline_pos, self.bgzf)


class FastxFilesDeclined(CrassError):
    """crass_hip_load_fastx_files declined a file (status 2, nothing resident): `layout` says which and why."""

    def __init__(self, status, where, layout):
        super().__init__(status, where)
        self.layout = layout


def _files_args(bufs):
    arrs = [_bytes_arg(b) for b in bufs]
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[(a.ctypes.data if len(a) else None) for a in arrs])
    lens = np.array([len(a) for a in arrs], dtype=np.uint64)
    return arrs, ptrs, lens


def fastx_files_scan_host(bufs, fastq_class=0):
    """Several files' bytes as one read set on the host (crass_fastx_files_scan_host; no GPU needed): a FastxFilesLayout,
    accepted or declined — what SearchEngine.load_fastx_files is tested against.  fastq_class 1: every FASTQ file by the
    wrapped rule (crass_fastx_files_scan_host_class)."""
    lib = _abi.load()
    arrs, ptrs, lens = _files_args(bufs)
    v = _abi.FastxFilesLayoutC()
    if fastq_class:
        st = lib.crass_fastx_files_scan_host_class(ptrs, lens.ctypes.data_as(_abi.u64p), len(arrs), int(fastq_class), C.byref(v))
    else:
        st = lib.crass_fastx_files_scan_host(ptrs, lens.ctypes.data_as(_abi.u64p), len(arrs), C.byref(v))
    try:
        if st not in (0, 2):
            raise CrassError(st, "crass_fastx_files_scan_host")
        return FastxFilesLayout(v)
    finally:
        lib.crass_fastx_files_layout_free(C.byref(v))


class FastxShards:
    """The files of a job cut into record-aligned shards (crass_fastx_shards), as numpy copies: n_ranks, n_files, n_reads,
    max_len, rank_read_base (uint64, n_ranks + 1), cut_file / cut_pos (n_ranks + 1: the file and the text position inside it
    of every actual cut), file_read_base (uint64, n_files + 1), formats.  A declined set has accepted False and the decline
    fields of a FastxFilesLayout, and empty arrays."""

    def __init__(self, v):
        self.n_ranks, self.n_files, self.n_reads, self.max_len = int(v.n_ranks), int(v.n_files), int(v.n_reads), int(v.max_len)
        self.decline_file, self.decline_reason, self.decline_pos = int(v.decline_file), int(v.decline_reason), int(v.decline_pos)
        self.bgzf = (int(v.bgzf.reason), int(v.bgzf.member), int(v.bgzf.in_pos))
        self.accepted = self.decline_file < 0
        have = bool(v.rank_read_base) and bool(v.cut_file) and bool(v.cut_pos) and bool(v.file_read_base) and bool(v.format)
        z = np.zeros(0, np.uint64)
        self.rank_read_base = _np(v.rank_read_base, self.n_ranks + 1, np.uint64).copy() if have else z
        self.cut_file = _np(v.cut_file, self.n_ranks + 1, np.uint32).copy() if have else np.zeros(0, np.uint32)
        self.cut_pos = _np(v.cut_pos, self.n_ranks + 1, np.uint64).copy() if have else z
        self.file_read_base = _np(v.file_read_base, self.n_files + 1, np.uint64).copy() if have else z
        self.formats = [bytes([int(v.format[f]) & 0xFF]) for f in range(self.n_files)] if have else []

    @property
    def verdict(self):
        """what a declined set is compared by: (file, FASTA / FASTQ reason, position, BGZF verdict)"""
        return (self.decline_file, self.decline_reason, self.decline_pos, self.bgzf)

    @property
    def cuts(self):
        """the actual cuts as a list of (file, position)"""
        return [(int(f), int(p)) for f, p in zip(self.cut_file, self.cut_pos)]


def _nominal_arg(nominal, n_ranks):
    if nominal is None:
        return None
    a = np.ascontiguousarray(nominal, dtype=np.uint64).reshape(-1)
    if len(a) != n_ranks - 1:
        raise ValueError("nominal needs n_ranks - 1 cuts")
    return a


def fastx_files_shards_host_gzip(files, n_ranks, nominal=None, fastq_class=0, gzip_mode=1, chunk_bytes=0):
    """fastx_files_shards_host for a job whose plain gzip files are taken as their text (crass_fastx_files_shards_host_gzip; no
    GPU needed): gzip_mode 0 is fastx_files_shards_host, the decline of plain gzip included; else such a file is
    gzip_inflate_host's text (chunk_bytes: 0 the default chunk), and one that does not inflate is the job's decline; gzip_mode 2:
    gzip_inflate_members_host's text, a file of any number of members."""
    lib = _abi.load()
    arrs, ptrs, lens = _files_args(files)
    nom = _nominal_arg(nominal, int(n_ranks))
    v = _abi.FastxShardsC()
    st = lib.crass_fastx_files_shards_host_gzip(ptrs, lens.ctypes.data_as(_abi.u64p), len(arrs), int(n_ranks),
                                                nom.ctypes.data if nom is not None and len(nom) else None, int(fastq_class), int(gzip_mode),
                                                int(chunk_bytes), C.byref(v))
    try:
        if st not in (0, 2):
            raise CrassError(st, "crass_fastx_files_shards_host_gzip")
        return FastxShards(v)
    finally:
        lib.crass_fastx_shards_free(C.byref(v))


def fastx_files_shards_host(files, n_ranks, nominal=None, fastq_class=0):
    """Several files' bytes cut into n_ranks record-aligned shards on the host (crass_fastx_files_shards_host_class; no GPU
    needed): a FastxShards, accepted or declined — what SearchGroup.load_fastx_files is tested against.  nominal: n_ranks - 1
    non-decreasing positions in the job's text space (None: even cuts).  fastq_class 1: a FASTQ file's record starts are those
    of the records the wrapped rule walks from line 0 (SearchGroup.set_fastq_class)."""
    lib = _abi.load()
    arrs, ptrs, lens = _files_args(files)
    nom = _nominal_arg(nominal, int(n_ranks))
    v = _abi.FastxShardsC()
    st = lib.crass_fastx_files_shards_host_class(ptrs, lens.ctypes.data_as(_abi.u64p), len(arrs), int(n_ranks),
                                                 nom.ctypes.data if nom is not None and len(nom) else None, int(fastq_class), C.byref(v))
    try:
        if st not in (0, 2):
            raise CrassError(st, "crass_fastx_files_shards_host_class")
        return FastxShards(v)
    finally:
        lib.crass_fastx_shards_free(C.byref(v))


def fastx_cut_probe_host(buf, left_is_ls):
    """The probe of a byte range on the host (crass_fastx_cut_probe_host): uint64 [7] — '\\n' bytes, line starts listed (at most 4),
    the first four line starts, the first line start whose byte is '>'; ~0 where there is none."""
    a = _bytes_arg(buf)
    out = np.zeros(7, np.uint64)
    _chk(_abi.load().crass_fastx_cut_probe_host(a.ctypes.data if len(a) else None, len(a), 1 if left_is_ls else 0, out.ctypes.data),
         "crass_fastx_cut_probe_host")
    return out


def fastx_header_ids(buf, rec_pos):
    """header_id[r] = index of the first read with the same name, from the file's bytes and the records' positions
    (crass_fastx_header_ids; host, names compared exactly).  rec_pos: n_reads + 1 entries as in a FastxLayout."""
    a = _bytes_arg(buf)
    rp = np.ascontiguousarray(rec_pos, dtype=np.uint64)
    n = max(len(rp) - 1, 0)
    out = np.zeros(n, np.uint64)
    _chk(_abi.load().crass_fastx_header_ids(a.ctypes.data if len(a) else None, len(a), rp.ctypes.data, n, out.ctypes.data),
         "crass_fastx_header_ids")
    return out


def _names_arg(names):
    """a list of names (bytes), or (uint8 array, uint64 offsets[n + 1]) -> (chars, offsets), contiguous"""
    if isinstance(names, tuple):
        chars, off = names
        return np.ascontiguousarray(chars, dtype=np.uint8).reshape(-1), np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
    return concat([bytes(x) for x in names])


def find_names(buf, rec_pos, names):
    """first[k] = the smallest record index whose NAME equals names[k] byte for byte, _abi.NAME_NOT_FOUND where there is none,
    from the file's bytes and the records' positions (crass_fastx_find_names; host).  rec_pos: n_reads + 1 entries as in a
    FastxLayout; names: a list of bytes, or (uint8 chars, uint64 offsets[n + 1]).  Returns uint64 [n]."""
    a = _bytes_arg(buf)
    rp = np.ascontiguousarray(rec_pos, dtype=np.uint64)
    n = max(len(rp) - 1, 0)
    chars, off = _names_arg(names)
    m = max(len(off) - 1, 0)
    out = np.zeros(m, np.uint64)
    _chk(_abi.load().crass_fastx_find_names(a.ctypes.data if len(a) else None, len(a), rp.ctypes.data if len(rp) else None, n,
                                            chars.ctypes.data if len(chars) else None, off.ctypes.data if len(off) else None, m,
                                            out.ctypes.data if m else None), "crass_fastx_find_names")
    return out


def names_of(buf, rec_pos, idx, idx_base=0, cap_bytes=None, out=None):
    """The NAMES of the records idx[k] - idx_base (any order, repeats allowed) back to back, from the file's bytes and the records'
    positions (crass_fastx_names_of; host): the statement of the rule SearchEngine.names_of_device is tested against.  rec_pos:
    n_reads + 1 entries as in a FastxLayout.  Returns (chars uint8, off uint64 [n + 1]).  cap_bytes / out: the capacity and the
    buffer to write into (tests: an overflow raises CrassError with status 8, its `offsets` complete and out filled up to the cap)."""
    a = _bytes_arg(buf)
    rp = np.ascontiguousarray(rec_pos, dtype=np.uint64)
    n = max(len(rp) - 1, 0)
    ix = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
    off = np.zeros(len(ix) + 1, np.uint64)
    lib = _abi.load()
    args = (a.ctypes.data if len(a) else None, len(a), rp.ctypes.data if len(rp) else None, n, ix.ctypes.data if len(ix) else None, len(ix), int(idx_base))
    if out is None and cap_bytes is None:          # measure, then fill
        st = lib.crass_fastx_names_of(*args, None, 0, off.ctypes.data)
        if st not in (0, _abi.ERR_OVERFLOW):
            _chk(st, "crass_fastx_names_of")
        cap_bytes = int(off[len(ix)])
    if out is None:
        out = np.zeros(int(cap_bytes), np.uint8)
    cap = len(out) if cap_bytes is None else int(cap_bytes)
    st = lib.crass_fastx_names_of(*args, out.ctypes.data if cap else None, cap, off.ctypes.data)
    if st != 0:
        e = CrassError(st, "crass_fastx_names_of")
        e.offsets = off
        raise e
    return out[:int(off[len(ix)])], off


def comments_of(buf, rec_pos, idx, file_read_base=None, idx_base=0, cap_bytes=None, out=None):
    """The comment kseq HANDS to the records idx[k] - idx_base (any order, repeats allowed): the own comment of the last record at
    or in front of it in the same file that has one (crass_fastx_comments_of; host) — the statement of the rule
    SearchEngine.fetch_comments is tested against.  rec_pos: n_reads + 1 entries as in a FastxLayout; file_read_base: n_files + 1
    read bases (None: one file), the bytes of several files in the arena layout (a '\n' behind each).  Returns (chars uint8, off
    uint64 [n + 1], has uint8 [n]).  cap_bytes / out: the capacity and the buffer to write into (tests: an overflow raises
    CrassError with status 8, its `offsets` and `has` complete and out filled up to the cap)."""
    a = _bytes_arg(buf)
    rp = np.ascontiguousarray(rec_pos, dtype=np.uint64)
    n = max(len(rp) - 1, 0)
    fb = None if file_read_base is None else np.ascontiguousarray(file_read_base, dtype=np.uint64)
    ix = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
    off = np.zeros(len(ix) + 1, np.uint64)
    has = np.zeros(len(ix), np.uint8)
    lib = _abi.load()
    args = (a.ctypes.data if len(a) else None, len(a), rp.ctypes.data if len(rp) else None, n, None if fb is None else fb.ctypes.data,
            0 if fb is None else len(fb) - 1, ix.ctypes.data if len(ix) else None, len(ix), int(idx_base))
    tail = (off.ctypes.data, has.ctypes.data if len(ix) else None)
    if out is None and cap_bytes is None:          # measure, then fill
        st = lib.crass_fastx_comments_of(*args, None, 0, *tail)
        if st not in (0, _abi.ERR_OVERFLOW):
            _chk(st, "crass_fastx_comments_of")
        cap_bytes = int(off[len(ix)])
    if out is None:
        out = np.zeros(int(cap_bytes), np.uint8)
    cap = len(out) if cap_bytes is None else int(cap_bytes)
    st = lib.crass_fastx_comments_of(*args, out.ctypes.data if cap else None, cap, *tail)
    if st != 0:
        e = CrassError(st, "crass_fastx_comments_of")
        e.offsets, e.has = off, has
        raise e
    return out[:int(off[len(ix)])], off, has


def _device_array(x, dtype, what):
    """(address, elements) of device memory: a raw address with its element count as a tuple (addr, n), or a contiguous torch
    device tensor of that dtype"""
    if isinstance(x, tuple):
        return (int(x[0]) or None), int(x[1])
    if str(x.dtype) != "torch." + dtype or not x.is_cuda or not x.is_contiguous():
        raise ValueError("%s: a contiguous %s device tensor or (address, elements)" % (what, dtype))
    return (int(x.data_ptr()) if x.numel() else None), int(x.numel())


class FastxFile:
    """FASTA/FASTQ(.gz) records with kseq_read semantics (C++ reader, crass_read_fastx)."""

    def __init__(self, path):
        lib = _abi.load()
        f = _abi.Fastx()
        _chk(lib.crass_read_fastx(str(path).encode(), C.byref(f)), "crass_read_fastx(%s)" % path)
        n = int(f.n_reads)
        self.n_reads = n
        self.max_len = int(f.max_len)
        self.last_ret = int(f.last_ret)
        self.seq_off = _np(f.seq_off, n + 1, np.uint64)
        self.seq = _np(f.seq, int(self.seq_off[-1]), np.uint8)
        self.name_off = _np(f.name_off, n + 1, np.uint64)
        self.name = _np(f.name, int(self.name_off[-1]), np.uint8)
        self.comment_off = _np(f.comment_off, n + 1, np.uint64)
        self.comment = _np(f.comment, int(self.comment_off[-1]), np.uint8)
        self.has_comment = _np(f.has_comment, n, np.uint8)
        self.qual_off = _np(f.qual_off, n + 1, np.uint64)
        self.qual = _np(f.qual, int(self.qual_off[-1]), np.uint8)
        self.has_qual = _np(f.has_qual, n, np.uint8)
        self.header_id = _np(f.header_id, n, np.uint64)
        lib.crass_free_fastx(C.byref(f))

    def _field(self, buf, off, i):
        return buf[int(off[i]):int(off[i + 1])].tobytes()

    def record(self, i):
        return (self._field(self.name, self.name_off, i),
                self._field(self.comment, self.comment_off, i) if self.has_comment[i] else None,
                self._field(self.seq, self.seq_off, i),
                self._field(self.qual, self.qual_off, i) if self.has_qual[i] else None)

    def records(self):
        return [self.record(i) for i in range(self.n_reads)]

    def unique_headers(self):
        return bool(np.all(self.header_id == np.arange(self.n_reads, dtype=np.uint64)))


class FastxIndex:
    """crass_index_fastx(_files): the input(s) kept mapped (plain text) or inflated once (gzip), the reads 2-bit packed at once, the
    records' text parsed on request; a list of paths = one read set in (file, read) order with header ids across the files.
    Raises CrassError(status 2, unsupported) for files that mix records with / without comment or quality."""

    def __init__(self, path):
        self.lib = _abi.load()
        h = C.c_void_p()
        if isinstance(path, (list, tuple)):
            arr = (C.c_char_p * len(path))(*[str(p).encode() for p in path])
            _chk(self.lib.crass_index_fastx_files(arr, len(path), C.byref(h)), "crass_index_fastx_files(%s)" % (path,))
        else:
            _chk(self.lib.crass_index_fastx(str(path).encode(), C.byref(h)), "crass_index_fastx(%s)" % path)
        self.h = h
        self.reads = _abi.Reads()
        ml, lr = C.c_uint32(), C.c_int()
        _chk(self.lib.crass_fastx_index_reads(self.h, C.byref(self.reads), C.byref(ml), C.byref(lr)), "crass_fastx_index_reads")
        self.max_len, self.last_ret, self.n_reads = int(ml.value), int(lr.value), int(self.reads.n_reads)

    def layout(self):
        """the packed reads as python objects: dict(stride, uniform_len, words per read (list of arrays), lengths, exceptions, header_id)"""
        r = self.reads
        n = self.n_reads
        stride, uni = int(r.stride_words), int(r.uniform_len)
        lengths = np.full(n, uni, np.uint32) if uni else _npv(r.lengths, n, np.uint32).copy()
        if stride:
            words = _npv(r.packed, n * stride, np.uint32).reshape(n, stride).copy() if n else np.zeros((0, stride), np.uint32)
            per = [words[i, :(int(lengths[i]) + 15) // 16] for i in range(n)]
        else:
            off = _npv(r.word_off, n + 1, np.uint64)
            allw = _npv(r.packed, int(off[n]), np.uint32).copy() if n else np.zeros(0, np.uint32)
            per = [allw[int(off[i]):int(off[i]) + (int(lengths[i]) + 15) // 16] for i in range(n)]
        ne = int(r.n_exceptions)
        exc = {}
        if ne:
            er, eo = _npv(r.exc_read, ne, np.uint64), _npv(r.exc_off, ne + 1, np.uint64)
            eb = _npv(r.exc_bytes, int(eo[ne]), np.uint8)
            exc = {int(er[k]): eb[int(eo[k]):int(eo[k + 1])].tobytes() for k in range(ne)}
        hid = _npv(r.header_id, n, np.uint64).tolist() if r.header_id else list(range(n))
        return dict(stride=stride, uniform_len=uni, words=per, lengths=lengths.tolist(), exceptions=exc, header_id=hid)

    def fetch(self, idx):
        """records (name, comment | None, seq, qual | None) of the read indices idx, in that order"""
        a = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
        f = _abi.Fastx()
        _chk(self.lib.crass_fastx_index_fetch(self.h, a.ctypes.data, len(a), C.byref(f)), "crass_fastx_index_fetch")
        n = int(f.n_reads)
        so, no, co, qo = (_np(x, n + 1, np.uint64) for x in (f.seq_off, f.name_off, f.comment_off, f.qual_off))
        sq, nm = _np(f.seq, int(so[-1]), np.uint8), _np(f.name, int(no[-1]), np.uint8)
        cm, ql = _np(f.comment, int(co[-1]), np.uint8), _np(f.qual, int(qo[-1]), np.uint8)
        hc, hq = _np(f.has_comment, n, np.uint8), _np(f.has_qual, n, np.uint8)
        out = [(nm[int(no[i]):int(no[i + 1])].tobytes(), cm[int(co[i]):int(co[i + 1])].tobytes() if hc[i] else None,
                sq[int(so[i]):int(so[i + 1])].tobytes(), ql[int(qo[i]):int(qo[i + 1])].tobytes() if hq[i] else None) for i in range(n)]
        self.lib.crass_free_fastx(C.byref(f))
        return out

    def drop_text(self):
        """give the plain-text inputs' mappings back (crass_fastx_index_drop_text); later fetches read from the files"""
        self.lib.crass_fastx_index_drop_text(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.crass_fastx_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_fastx(path, chunk_bytes=0, with_names=True):
    """The records of a FASTA/FASTQ(.gz) file through the chunked reader (crass_fastx_stream_*): a list of (name, comment, seq, qual)
    like FastxFile.records(), the header ids (job-level index of the first read with the same name), kseq_read's final return value
    and the number of chunks it took."""
    lib = _abi.load()
    tab = C.c_void_p(lib.crass_name_table_create()) if with_names else C.c_void_p()
    h = C.c_void_p()
    _chk(lib.crass_fastx_stream_open(str(path).encode(), int(chunk_bytes), tab, 0, C.byref(h)), "crass_fastx_stream_open(%s)" % path)
    recs, hid, last, chunks = [], [], -1, 0
    try:
        while True:
            f = _abi.Fastx()
            _chk(lib.crass_fastx_stream_next(h, C.byref(f)), "crass_fastx_stream_next")
            last = int(f.last_ret)
            n = int(f.n_reads)
            if n == 0:
                break
            chunks += 1
            so, no = _np(f.seq_off, n + 1, np.uint64), _np(f.name_off, n + 1, np.uint64)
            co, qo = _np(f.comment_off, n + 1, np.uint64), _np(f.qual_off, n + 1, np.uint64)
            sq, nm = _np(f.seq, int(so[-1]), np.uint8), _np(f.name, int(no[-1]), np.uint8)
            cm, ql = _np(f.comment, int(co[-1]), np.uint8), _np(f.qual, int(qo[-1]), np.uint8)
            hc, hq = _np(f.has_comment, n, np.uint8), _np(f.has_qual, n, np.uint8)
            hid.extend(_np(f.header_id, n, np.uint64).tolist())
            for i in range(n):
                recs.append((nm[int(no[i]):int(no[i + 1])].tobytes(), cm[int(co[i]):int(co[i + 1])].tobytes() if hc[i] else None,
                             sq[int(so[i]):int(so[i + 1])].tobytes(), ql[int(qo[i]):int(qo[i + 1])].tobytes() if hq[i] else None))
        assert int(lib.crass_fastx_stream_reads_done(h)) == len(recs)
    finally:
        lib.crass_fastx_stream_close(h)
        if with_names:
            lib.crass_name_table_destroy(tab)
    return recs, hid, last, chunks


def synth_spec(**kw):
    s = _abi.SynthSpec()
    _abi.load().crass_synth_default(C.byref(s))
    for k, v in kw.items():
        if not hasattr(s, k):
            raise AttributeError(k)
        setattr(s, k, v)
    return s


def synth_packed(spec, first_read, n_reads, out=None, n_threads=0):
    """Deterministic synthetic reads [first_read, first_read+n_reads) as packed uint32 words
    (uniform stride ceil(L/16)).  `out` may be a preallocated (e.g. pinned) uint32 array."""
    W = (spec.read_len + 15) // 16
    if out is None:
        out = np.empty(int(n_reads) * W, dtype=np.uint32)
    assert out.dtype == np.uint32 and out.size >= int(n_reads) * W
    _chk(_abi.load().crass_synth_packed(C.byref(spec), int(first_read), int(n_reads), out.ctypes.data, int(n_threads)),
         "crass_synth_packed")
    return out


def unpack_ascii(packed, stride_words, read_len, n_reads):
    out = np.empty(int(n_reads) * int(read_len), dtype=np.uint8)
    _chk(_abi.load().crass_unpack_ascii(packed.ctypes.data, int(stride_words), int(read_len), int(n_reads),
                                        out.ctypes.data), "crass_unpack_ascii")
    return out


class CandidateSet:
    def __init__(self, v):
        n = int(v.n)
        self.n = n
        self.read_idx = _np(v.read_idx, n, np.uint64)
        self.low_lexi = _np(v.low_lexi, n, np.uint8)
        self.repeat_len = _np(v.repeat_len, n, np.uint32)
        self.n_ss = _np(v.n_ss, n, np.uint32)
        self.ss_off = _np(v.ss_off, n, np.uint64)
        # the pool may be fixed-stride slots (ss_off[k] = k*cap) or tightly packed: size it from the offsets
        pool_len = int((self.ss_off + self.n_ss).max()) if n else 0
        self.ss_pool = _np(v.ss_pool, pool_len, np.uint32)
        self.dr_stride = int(v.dr_stride)
        self.dr_len = _np(v.dr_len, n, np.uint16)
        self.dr_chars = _np(C.cast(v.dr_chars, _abi.u8p), n * self.dr_stride, np.uint8)
        self.max_read_len = int(v.max_read_len)

    def ss(self, k):
        o = int(self.ss_off[k])
        return self.ss_pool[o:o + int(self.n_ss[k])].tolist()

    def dr(self, k):
        o = k * self.dr_stride
        return self.dr_chars[o:o + int(self.dr_len[k])].tobytes()


class MergeResult:
    def __init__(self, v):
        self.n_tokens = int(v.n_tokens)
        self.tok_off = _np(v.tok_off, self.n_tokens + 1, np.uint64)
        tc = C.string_at(v.tok_chars, int(self.tok_off[-1])) if self.n_tokens else b""
        self.tokens = [tc[int(self.tok_off[i]):int(self.tok_off[i + 1])] for i in range(self.n_tokens)]
        self.cand_token = _np(v.cand_token, int(v.n_candidates), np.uint32)
        self.n_groups = int(v.n_groups)
        self.grp_off = _np(v.grp_off, self.n_groups + 1, np.uint64)
        gt = _np(v.grp_tokens, int(self.grp_off[-1]) if self.n_groups else 0, np.uint32)
        self.groups = [gt[int(self.grp_off[i]):int(self.grp_off[i + 1])].tolist() for i in range(self.n_groups)]
        self.n_patterns = int(v.n_patterns)
        self.pat_off = _np(v.pat_off, self.n_patterns + 1, np.uint64)
        pc = C.string_at(v.pat_chars, int(self.pat_off[-1])) if self.n_patterns else b""
        self.patterns = [pc[int(self.pat_off[i]):int(self.pat_off[i + 1])] for i in range(self.n_patterns)]
        self.pat_group = _np(v.pat_group, self.n_patterns, np.uint32)
        self.next_free_gid = int(v.next_free_gid)


def merge_host(dr_chars, dr_len, kmer_clust_size=6):
    """createNonRedundantSet on the host without a GPU context (crass_merge_create).
    dr_chars: uint8 [n, stride]; dr_len: uint16 [n]."""
    lib = _abi.load()
    dr_chars = np.ascontiguousarray(dr_chars, dtype=np.uint8)
    dr_len = np.ascontiguousarray(dr_len, dtype=np.uint16)
    n = dr_chars.shape[0]
    stride = dr_chars.shape[1] if dr_chars.ndim == 2 and n else 16
    h = C.c_void_p()
    _chk(lib.crass_merge_create(dr_chars.ctypes.data, dr_len.ctypes.data, int(stride), int(n), int(kmer_clust_size),
                                C.byref(h)), "crass_merge_create")
    try:
        v = _abi.MergeView()
        _chk(lib.crass_merge_get(h, C.byref(v)), "crass_merge_get")
        return MergeResult(v)
    finally:
        lib.crass_merge_destroy(h)


def merge_rebuild(dx_chars, dx_len, cand_distinct, gid_of, dropped, n_groups):
    """host view of a merge from per-token results (crass_merge_rebuild): what the engine does after the device
    merge, callable without a GPU.  dx_chars: uint8 [n_distinct, stride] in token order."""
    lib = _abi.load()
    dx_chars = np.ascontiguousarray(dx_chars, dtype=np.uint8)
    dx_len = np.ascontiguousarray(dx_len, dtype=np.uint16)
    cand = np.ascontiguousarray(cand_distinct, dtype=np.uint32)
    gid = np.ascontiguousarray(gid_of, dtype=np.uint32)
    drop = np.ascontiguousarray(dropped, dtype=np.uint8)
    nd = dx_chars.shape[0]
    stride = dx_chars.shape[1] if nd else 16
    h = C.c_void_p()
    _chk(lib.crass_merge_rebuild(dx_chars.ctypes.data, dx_len.ctypes.data, int(stride), int(nd), cand.ctypes.data, int(len(cand)),
                                 gid.ctypes.data, drop.ctypes.data, int(n_groups), C.byref(h)), "crass_merge_rebuild")
    try:
        v = _abi.MergeView()
        _chk(lib.crass_merge_get(h, C.byref(v)), "crass_merge_get")
        return MergeResult(v)
    finally:
        lib.crass_merge_destroy(h)


def dr_slots(strings, stride=48):
    """list[bytes] -> (uint8 [n, stride], uint16 [n]) in the C ABI's fixed-slot layout"""
    n = len(strings)
    chars = np.zeros((n, stride), np.uint8)
    lens = np.zeros(n, np.uint16)
    for i, s in enumerate(strings):
        chars[i, :len(s)] = np.frombuffer(s, np.uint8)
        lens[i] = len(s)
    return chars, lens


class RecruitSet:
    def __init__(self, v):
        n = int(v.n)
        self.n = n
        self.read_idx = _np(v.read_idx, n, np.uint64)
        self.low_lexi = _np(v.low_lexi, n, np.uint8)
        self.start = _np(v.start, n, np.uint32)
        self.end = _np(v.end, n, np.uint32)
        self.dr_stride = int(v.dr_stride)
        self.dr_len = _np(v.dr_len, n, np.uint16)
        self.dr_chars = _np(C.cast(v.dr_chars, _abi.u8p), n * self.dr_stride, np.uint8)
        self.token = _np(v.token, n, np.uint32)

    def dr(self, k):
        o = k * self.dr_stride
        return self.dr_chars[o:o + int(self.dr_len[k])].tobytes()


class SearchEngine:
    """One context per GPU (crass_hip_create).  Call order mirrors WorkHorse::parseSeqFiles
    (WorkHorse.cpp:321-414): load_reads -> seed_scan (searchFile) -> merge
    (createNonRedundantSet) -> recruit (findSingletons)."""

    def __init__(self, params=None, device=0):
        self.lib = _abi.load()
        self.params = params or default_params()
        h = C.c_void_p()
        _chk(self.lib.crass_hip_create(C.byref(self.params), int(device), C.byref(h)), "crass_hip_create")
        self.h = h
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.crass_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- reads ----
    def load_reads(self, packed, header_id=None, read_index_base=0):
        r = _abi.Reads()
        C.memmove(C.byref(r), C.byref(packed.reads), C.sizeof(r))
        hid = None
        if header_id is not None:
            hid = np.ascontiguousarray(header_id, dtype=np.uint64)
            r.header_id = hid.ctypes.data
        r.read_index_base = int(read_index_base)
        _chk(self.lib.crass_hip_load_reads(self.h, C.byref(r)), "crass_hip_load_reads")
        self._keep = (packed, hid)

    def load_packed_uniform(self, words, n_reads, read_len, read_index_base=0):
        """Host uint32 array of uniform-stride packed reads (synthetic generator output)."""
        r = _abi.Reads()
        r.n_reads = int(n_reads)
        r.packed = words.ctypes.data
        r.stride_words = (int(read_len) + 15) // 16
        r.uniform_len = int(read_len)
        r.read_index_base = int(read_index_base)
        _chk(self.lib.crass_hip_load_reads(self.h, C.byref(r)), "crass_hip_load_reads")

    def attach_device_tensor(self, tensor, n_reads, read_len, read_index_base=0):
        """Zero-copy: a torch int32 CUDA tensor holding uniform-stride packed reads."""
        r = _abi.Reads()
        r.n_reads = int(n_reads)
        r.packed = int(tensor.data_ptr())
        r.stride_words = (int(read_len) + 15) // 16
        r.uniform_len = int(read_len)
        r.read_index_base = int(read_index_base)
        _chk(self.lib.crass_hip_attach_device_reads(self.h, C.byref(r)), "crass_hip_attach_device_reads")
        self._keep = tensor

    @staticmethod
    def _text_args(seqs):
        # a (buffer, offsets) pair: two elements, the second an array of offsets (not a read); anything else: a list of reads
        if isinstance(seqs, tuple) and len(seqs) == 2 and not isinstance(seqs[1], (bytes, bytearray)):
            buf, off = seqs
            if isinstance(buf, (bytes, bytearray)):
                buf = np.frombuffer(bytes(buf), dtype=np.uint8)
            return buf, np.ascontiguousarray(off, dtype=np.uint64)
        return concat(list(seqs))

    def load_text(self, seqs, pad_uniform=2, header_id=None, read_index_base=0):
        """Sequence text (a list of bytes, or a (uint8 buffer, offsets[n + 1]) pair) in host memory; packed on the
        device (crass_hip_load_text).  The state afterwards is that of load_reads(PackedReads(seqs, pad_uniform))."""
        buf, off = self._text_args(seqs)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        hid = None if header_id is None else np.ascontiguousarray(header_id, dtype=np.uint64)
        _chk(self.lib.crass_hip_load_text(self.h, buf.ctypes.data, off.ctypes.data, len(off) - 1, int(pad_uniform),
                                          None if hid is None else hid.ctypes.data, int(read_index_base)), "crass_hip_load_text")
        self._keep = None

    def attach_device_text(self, tensor, offsets, pad_uniform=2, header_id=None, read_index_base=0):
        """Sequence text in a torch uint8 DEVICE tensor (offsets[n + 1]: host array of byte offsets into it); packed on
        the device (crass_hip_attach_device_text).  The context keeps nothing of the tensor."""
        if str(tensor.dtype) != "torch.uint8" or not tensor.is_cuda or not tensor.is_contiguous():
            raise ValueError("attach_device_text needs a contiguous uint8 device tensor")
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(off) > 1 and int(off[-1]) > tensor.numel():
            raise ValueError("offsets reach beyond the tensor")
        hid = None if header_id is None else np.ascontiguousarray(header_id, dtype=np.uint64)
        _chk(self.lib.crass_hip_attach_device_text(self.h, int(tensor.data_ptr()), off.ctypes.data, len(off) - 1, int(pad_uniform),
                                                   None if hid is None else hid.ctypes.data, int(read_index_base)),
             "crass_hip_attach_device_text")
        self._keep = None

    def last_pack_ms(self):
        """HIP-event milliseconds of the last load_text / attach_device_text call's pack kernels (stage timing >= 1, else 0)."""
        return float(self.lib.crass_hip_last_pack_ms(self.h))

    def _fastx_result(self, st, v, where):
        lay = FastxLayout(v)
        if st == 2 and lay.decline_reason:
            raise FastxDeclined(st, where, lay)
        _chk(st, where)
        self._keep = None
        return lay

    def load_fastx_bytes(self, buf, pad_uniform=2, read_index_base=0):
        """The raw bytes of a FASTA / FASTQ file in host memory (bytes or a uint8 array); records found and reads packed on the
        device (crass_hip_load_fastx_bytes).  Returns a FastxLayout; raises FastxDeclined (status 2, nothing resident) for an
        input outside the regular class.  Header ids: set_header_ids(fastx_header_ids(buf, layout.rec_pos))."""
        a = _bytes_arg(buf)
        v = _abi.FastxLayoutC()
        st = self.lib.crass_hip_load_fastx_bytes(self.h, a.ctypes.data if len(a) else None, len(a), int(pad_uniform), int(read_index_base),
                                                 C.byref(v))
        return self._fastx_result(st, v, "crass_hip_load_fastx_bytes")

    def attach_device_fastx(self, tensor, pad_uniform=2, read_index_base=0):
        """The same for file bytes in a torch uint8 DEVICE tensor of any alignment (crass_hip_attach_device_fastx).  The context
        keeps nothing of the tensor."""
        if str(tensor.dtype) != "torch.uint8" or not tensor.is_cuda or not tensor.is_contiguous():
            raise ValueError("attach_device_fastx needs a contiguous uint8 device tensor")
        v = _abi.FastxLayoutC()
        st = self.lib.crass_hip_attach_device_fastx(self.h, int(tensor.data_ptr()) if tensor.numel() else None, int(tensor.numel()),
                                                    int(pad_uniform), int(read_index_base), C.byref(v))
        return self._fastx_result(st, v, "crass_hip_attach_device_fastx")

    def inflate_bgzf_device(self, tensor_in, index, tensor_out):
        """The members of a BGZF file whose bytes are in a torch uint8 DEVICE tensor (any alignment), inflated on the device into
        tensor_out (the same; at least index.n_text bytes): crass_hip_inflate_bgzf_device.  index: the BgzfIndex of the same bytes.
        Returns the bytes of text; raises BgzfDeclined with the host function's verdict.  The resident set is untouched."""
        for t in (tensor_in, tensor_out):
            if str(t.dtype) != "torch.uint8" or not t.is_cuda or not t.is_contiguous():
                raise ValueError("inflate_bgzf_device needs contiguous uint8 device tensors")
        ver = _abi.BgzfVerdict()
        ixc = index._c()
        st = self.lib.crass_hip_inflate_bgzf_device(self.h, int(tensor_in.data_ptr()) if tensor_in.numel() else None, int(tensor_in.numel()), C.byref(ixc),
                                                    int(tensor_out.data_ptr()) if tensor_out.numel() else None, int(tensor_out.numel()), C.byref(ver))
        if st == 2:
            raise BgzfDeclined(st, "crass_hip_inflate_bgzf_device", ver)
        _chk(st, "crass_hip_inflate_bgzf_device")
        return index.n_text

    def load_fastx_bgzf(self, buf, pad_uniform=2, read_index_base=0, keep=None):
        """The bytes of a BGZF-compressed FASTA / FASTQ file in host memory: indexed on the host, inflated, scanned and packed on
        the device (crass_hip_load_fastx_bgzf).  Returns a FastxLayout, as attach_device_fastx on the inflated bytes would; raises
        BgzfDeclined (the compression) or FastxDeclined (the text), nothing resident either way.  keep: a contiguous torch uint8
        DEVICE tensor of at least the text's size — the text stays in its first layout.rec_pos[-1] bytes, for device_header_ids
        and fetch_header_lines."""
        a = _bytes_arg(buf)
        if keep is not None and (str(keep.dtype) != "torch.uint8" or not keep.is_cuda or not keep.is_contiguous()):
            raise ValueError("load_fastx_bgzf(keep=...) needs a contiguous uint8 device tensor")
        v, ver = _abi.FastxLayoutC(), _abi.BgzfVerdict()
        st = self.lib.crass_hip_load_fastx_bgzf(self.h, a.ctypes.data if len(a) else None, len(a), int(pad_uniform), int(read_index_base),
                                                int(keep.data_ptr()) if keep is not None and keep.numel() else None,
                                                int(keep.numel()) if keep is not None else 0, C.byref(v), C.byref(ver))
        if st == 2 and ver.reason:
            raise BgzfDeclined(st, "crass_hip_load_fastx_bgzf", ver)
        return self._fastx_result(st, v, "crass_hip_load_fastx_bgzf")

    def inflate_gzip_device(self, tensor_in, tensor_out, chunk_bytes=0, with_plan=False):
        """A plain (single-member) gzip file whose bytes are in a torch uint8 DEVICE tensor (any alignment), inflated on the device
        chunk by chunk into tensor_out (the same): crass_hip_inflate_gzip_device.  Returns the bytes of text, with with_plan
        (n_text, GzipPlan); raises BgzfDeclined with the host function's verdict (`plan`: the GzipPlan when the header parsed);
        a tensor_out too small raises CrassError with status 8 and the text's size in its `n_text`, nothing written.  The
        resident set is untouched."""
        for t in (tensor_in, tensor_out):
            if str(t.dtype) != "torch.uint8" or not t.is_cuda or not t.is_contiguous():
                raise ValueError("inflate_gzip_device needs contiguous uint8 device tensors")
        n_text, ver, pc = C.c_uint64(0), _abi.BgzfVerdict(), _abi.GzipPlanC()
        try:
            st = self.lib.crass_hip_inflate_gzip_device(self.h, int(tensor_in.data_ptr()) if tensor_in.numel() else None, int(tensor_in.numel()),
                                                        int(chunk_bytes), int(tensor_out.data_ptr()) if tensor_out.numel() else None,
                                                        int(tensor_out.numel()), C.byref(n_text), C.byref(pc), C.byref(ver))
            plan = GzipPlan(pc)
        finally:
            self.lib.crass_gzip_plan_free(C.byref(pc))
        if st == 2:
            e = BgzfDeclined(st, "crass_hip_inflate_gzip_device", ver)
            e.plan = plan
            raise e
        if st == 8:
            e = CrassError(st, "crass_hip_inflate_gzip_device")
            e.n_text, e.plan = int(n_text.value), plan
            raise e
        _chk(st, "crass_hip_inflate_gzip_device")
        return (int(n_text.value), plan) if with_plan else int(n_text.value)

    def inflate_gzip_members_device(self, tensor_in, tensor_out, chunk_bytes=0, with_plan=False):
        """inflate_gzip_device for a plain gzip file of any number of members (crass_hip_inflate_gzip_members_device).  Returns the
        bytes of text, with with_plan (n_text, GzipPlan, GzipMembers); raises as inflate_gzip_device does, with the verdict of
        gzip_inflate_members_host."""
        for t in (tensor_in, tensor_out):
            if str(t.dtype) != "torch.uint8" or not t.is_cuda or not t.is_contiguous():
                raise ValueError("inflate_gzip_members_device needs contiguous uint8 device tensors")
        fn = "crass_hip_inflate_gzip_members_device"
        n_text, ver, pc, mc = C.c_uint64(0), _abi.BgzfVerdict(), _abi.GzipPlanC(), _abi.GzipMembersC()
        try:
            st = self.lib.crass_hip_inflate_gzip_members_device(self.h, int(tensor_in.data_ptr()) if tensor_in.numel() else None,
                                                                int(tensor_in.numel()), int(chunk_bytes),
                                                                int(tensor_out.data_ptr()) if tensor_out.numel() else None,
                                                                int(tensor_out.numel()), C.byref(n_text), C.byref(pc), C.byref(mc), C.byref(ver))
            plan, members = GzipPlan(pc), GzipMembers(mc)
        finally:
            self.lib.crass_gzip_plan_free(C.byref(pc))
            self.lib.crass_gzip_members_free(C.byref(mc))
        if st == 2:
            e = BgzfDeclined(st, fn, ver)
            e.plan = plan
            raise e
        if st == 8:
            e = CrassError(st, fn)
            e.n_text, e.plan = int(n_text.value), plan
            raise e
        _chk(st, fn)
        return (int(n_text.value), plan, members) if with_plan else int(n_text.value)

    def load_fastx_gzip_members(self, buf, pad_uniform=2, read_index_base=0, keep=None, with_members=False):
        """load_fastx_gzip for a plain gzip file of any number of members (crass_hip_load_fastx_gzip_members); with with_members
        (layout, GzipMembers)."""
        a = _bytes_arg(buf)
        if keep is not None and (str(keep.dtype) != "torch.uint8" or not keep.is_cuda or not keep.is_contiguous()):
            raise ValueError("load_fastx_gzip_members(keep=...) needs a contiguous uint8 device tensor")
        v, ver, mc = _abi.FastxLayoutC(), _abi.BgzfVerdict(), _abi.GzipMembersC()
        try:
            st = self.lib.crass_hip_load_fastx_gzip_members(self.h, a.ctypes.data if len(a) else None, len(a), int(pad_uniform), int(read_index_base),
                                                            int(keep.data_ptr()) if keep is not None and keep.numel() else None,
                                                            int(keep.numel()) if keep is not None else 0, C.byref(v), C.byref(mc), C.byref(ver))
            members = GzipMembers(mc)
        finally:
            self.lib.crass_gzip_members_free(C.byref(mc))
        if st == 2 and ver.reason:
            raise BgzfDeclined(st, "crass_hip_load_fastx_gzip_members", ver)
        lay = self._fastx_result(st, v, "crass_hip_load_fastx_gzip_members")
        return (lay, members) if with_members else lay

    def load_fastx_gzip(self, buf, pad_uniform=2, read_index_base=0, keep=None):
        """The bytes of a plain gzip FASTA / FASTQ file in host memory: inflated chunk by chunk, scanned and packed on the device
        (crass_hip_load_fastx_gzip), the mirror of load_fastx_bgzf."""
        a = _bytes_arg(buf)
        if keep is not None and (str(keep.dtype) != "torch.uint8" or not keep.is_cuda or not keep.is_contiguous()):
            raise ValueError("load_fastx_gzip(keep=...) needs a contiguous uint8 device tensor")
        v, ver = _abi.FastxLayoutC(), _abi.BgzfVerdict()
        st = self.lib.crass_hip_load_fastx_gzip(self.h, a.ctypes.data if len(a) else None, len(a), int(pad_uniform), int(read_index_base),
                                                int(keep.data_ptr()) if keep is not None and keep.numel() else None,
                                                int(keep.numel()) if keep is not None else 0, C.byref(v), C.byref(ver))
        if st == 2 and ver.reason:
            raise BgzfDeclined(st, "crass_hip_load_fastx_gzip", ver)
        return self._fastx_result(st, v, "crass_hip_load_fastx_gzip")

    def set_gzip_on_device(self, on=True, members=False):
        """load_fastx_files takes a plain gzip file on a BGZF file's terms (crass_hip_set_gzip_on_device); default off.  members:
        plain gzip of any number of members (CRASS_GZIP_ON_DEVICE_MEMBERS), else single-member files only."""
        _chk(self.lib.crass_hip_set_gzip_on_device(self.h, (2 if members else 1) if on else 0), "crass_hip_set_gzip_on_device")

    def set_fastq_class(self, fastq_class):
        """The class the device ingest reads FASTQ by (crass_hip_set_fastq_class): 0, the default, the four-line form only; 1 also
        wrapped FASTQ — records over several lines, blank lines between records and at the end."""
        _chk(self.lib.crass_hip_set_fastq_class(self.h, int(fastq_class)), "crass_hip_set_fastq_class")

    def last_scan_classes(self):
        """(pieces decided by the four-line scan, pieces decided by the wrapped scan) of the last device load
        (crass_hip_last_scan_classes)."""
        out = (C.c_uint64 * 2)()
        _chk(self.lib.crass_hip_last_scan_classes(self.h, out), "crass_hip_last_scan_classes")
        return int(out[0]), int(out[1])

    def last_gzip_ms(self):
        """HIP-event milliseconds of the last gzip inflate's steps: dict find, count, decode, windows, narrow (stage timing >= 1, else 0)."""
        ms = (C.c_float * 5)()
        _chk(self.lib.crass_hip_last_gzip_ms(self.h, ms), "crass_hip_last_gzip_ms")
        return dict(zip(("find", "count", "decode", "windows", "narrow"), (float(x) for x in ms)))

    def load_fastx_files(self, bufs, pad_uniform=2):
        """Several input files' bytes (plain FASTA / FASTQ or BGZF, each on its own terms) as ONE resident set in (file, read)
        order, parsed on the device, header ids across the files installed (crass_hip_load_fastx_files).  Returns a
        FastxFilesLayout; raises FastxFilesDeclined (status 2, nothing resident) when a file is declined.  The files' text stays
        on the device: resident_fastx()."""
        arrs, ptrs, lens = _files_args(bufs)
        v = _abi.FastxFilesLayoutC()
        st = self.lib.crass_hip_load_fastx_files(self.h, ptrs, lens.ctypes.data_as(_abi.u64p), len(arrs), int(pad_uniform), C.byref(v))
        lay = FastxFilesLayout(v)
        if st == 2 and not lay.accepted:
            raise FastxFilesDeclined(st, "crass_hip_load_fastx_files", lay)
        _chk(st, "crass_hip_load_fastx_files")
        self._keep = None
        return lay

    def cut_probe_device(self, src, n_bytes, left_is_ls):
        """fastx_cut_probe_host's answer for n_bytes bytes on the DEVICE (src: an address or a torch uint8 device tensor, any
        alignment), by k_fx_cut_probe (crass_hip_fastx_cut_probe_device).  last_cut_probe_ms(): the kernel's HIP-event time."""
        ptr = src if isinstance(src, int) else (int(src.data_ptr()) if src.numel() else 0)
        out = np.zeros(7, np.uint64)
        _chk(self.lib.crass_hip_fastx_cut_probe_device(self.h, ptr or None, int(n_bytes), 1 if left_is_ls else 0, out.ctypes.data),
             "crass_hip_fastx_cut_probe_device")
        return out

    def last_cut_probe_ms(self):
        return float(self.lib.crass_hip_last_cut_probe_ms(self.h))

    def last_cut_chain_ms(self):
        """HIP-event ms of the cut kernels (k_fw_summary .. k_fw_cut_jump) of this context's part of a group's last wrapped-mode
        files load (crass_hip_last_cut_chain_ms); measured at stage timing level >= 1, else 0."""
        return float(self.lib.crass_hip_last_cut_chain_ms(self.h))

    def resident_fastx(self):
        """(device address, n_bytes) of the arena of the last load_fastx_files (crass_hip_resident_fastx); CrassError with
        status CRASS_ERR_STATE when the last load was not one.  The address goes where fetch_quality takes `src`; for
        device_header_ids and fetch_header_lines (which take the byte count from rec_pos[-1] when src is an address) pass
        np.append(layout.rec_pos[:-1], n_bytes) as the layout."""
        p, n = C.c_void_p(), C.c_uint64()
        _chk(self.lib.crass_hip_resident_fastx(self.h, C.byref(p), C.byref(n)), "crass_hip_resident_fastx")
        return int(p.value or 0), int(n.value)

    def fetch_quality(self, src, n_bytes, rec_pos, idx, out=None):
        """The quality strings of the records idx (LOCAL record numbers, any order, repeats allowed) of file bytes on the DEVICE
        (src: an address or a contiguous torch uint8 device tensor; n_bytes: how many; rec_pos: n_reads + 1 positions):
        crass_hip_fetch_quality_device.  Returns (chars, off, has_qual): numpy copies of the strings back to back (uint8), their
        offsets (uint64, n + 1) and whether the record is a FASTQ one (uint8).  out: a contiguous torch uint8 DEVICE tensor — the
        strings are written there instead (crass_hip_fetch_quality_device_to) and chars is None; a tensor too small raises
        CrassError with status 8 and the offsets in its `offsets`."""
        ptr = src if isinstance(src, int) else (int(src.data_ptr()) if src.numel() else 0)
        rp = np.ascontiguousarray(rec_pos, dtype=np.uint64)
        n = max(len(rp) - 1, 0)
        a = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
        has = np.zeros(len(a), np.uint8)
        args = (self.h, ptr or None, int(n_bytes), rp.ctypes.data if n else None, n, a.ctypes.data if len(a) else None, len(a))
        if out is None:
            v = _abi.Text()
            _chk(self.lib.crass_hip_fetch_quality_device(*args, C.byref(v), has.ctypes.data if len(a) else None), "crass_hip_fetch_quality_device")
            t = Text(v)
            return t.chars.copy(), t.off.copy(), has
        if str(out.dtype) != "torch.uint8" or not out.is_cuda or not out.is_contiguous():
            raise ValueError("fetch_quality(out=...) needs a contiguous uint8 device tensor")
        off = np.zeros(len(a) + 1, np.uint64)
        st = self.lib.crass_hip_fetch_quality_device_to(*args, int(out.data_ptr()) if out.numel() else None, int(out.numel()), off.ctypes.data,
                                                        has.ctypes.data if len(a) else None)
        if st != 0:
            e = CrassError(st, "crass_hip_fetch_quality_device_to")
            e.offsets = off
            raise e
        return None, off, has

    def last_inflate_ms(self):
        """HIP-event milliseconds of the last inflate_bgzf_device / load_fastx_bgzf call's inflate kernel (stage timing >= 1, else 0)."""
        return float(self.lib.crass_hip_last_inflate_ms(self.h))

    def set_header_ids(self, arr):
        """header_id of the resident set (None: all headers unique), whichever call loaded it; drops earlier results as a load
        does (crass_hip_set_header_ids)."""
        hid = None if arr is None else np.ascontiguousarray(arr, dtype=np.uint64)
        _chk(self.lib.crass_hip_set_header_ids(self.h, None if hid is None else hid.ctypes.data), "crass_hip_set_header_ids")

    @staticmethod
    def _device_bytes(src, layout):
        """(address, n_bytes, rec_pos, n_reads) of file bytes on the device: src is a contiguous torch uint8 device tensor, or a
        raw device address (then the layout's rec_pos[n_reads] is the byte count); layout: a FastxLayout or its rec_pos"""
        rp = np.ascontiguousarray(getattr(layout, "rec_pos", layout), dtype=np.uint64)
        n = max(len(rp) - 1, 0)
        if isinstance(src, int):
            return (src or None), (int(rp[n]) if len(rp) else 0), rp, n
        if str(src.dtype) != "torch.uint8" or not src.is_cuda or not src.is_contiguous():
            raise ValueError("file bytes on the device: a contiguous uint8 device tensor or an address")
        return (int(src.data_ptr()) if src.numel() else None), int(src.numel()), rp, n

    def device_header_ids(self, src, layout, install=True):
        """header_id[r] = index of the first read with the same name, from file bytes that live on the DEVICE (a torch uint8
        tensor or an address) and the records' positions (a FastxLayout or its rec_pos): what fastx_header_ids gives on the
        same bytes, computed on the device (crass_hip_fastx_header_ids_device).  install: also make them the resident set's,
        as set_header_ids does, without a host round trip.  Returns (ids, n_repeated)."""
        ptr, nb, rp, n = self._device_bytes(src, layout)
        out = np.zeros(n, np.uint64)
        rep = C.c_uint64()
        _chk(self.lib.crass_hip_fastx_header_ids_device(self.h, ptr, nb, rp.ctypes.data if n else None, n, out.ctypes.data if n else None,
                                                        1 if install else 0, C.byref(rep)), "crass_hip_fastx_header_ids_device")
        return out, int(rep.value)

    def last_header_ids_ms(self):
        """HIP-event milliseconds of the last device_header_ids call: (all kernels, insert launches, lookup launch); stage
        timing >= 1, else zeros."""
        return tuple(float(self.lib.crass_hip_last_header_ids_ms(self.h, k)) for k in range(3))

    def names_build(self, src, layout):
        """Builds and KEEPS the name table of file bytes on the DEVICE (src, layout: as fetch_header_lines takes them) for
        names_find (crass_hip_fastx_names_build_device).  The table refers to the bytes: keep the tensor alive and unchanged
        until names_drop, the next names_build, or close.  names_build(None, None): the arena and layout of the last
        load_fastx_files; any load or attach then drops the table."""
        if src is None and layout is None:
            _chk(self.lib.crass_hip_fastx_names_build_device(self.h, None, 0, None, 0), "crass_hip_fastx_names_build_device")
            self._names_keep = None
            return
        ptr, nb, rp, n = self._device_bytes(src, layout)
        _chk(self.lib.crass_hip_fastx_names_build_device(self.h, ptr, nb, rp.ctypes.data, n), "crass_hip_fastx_names_build_device")
        self._names_keep = src

    def names_find(self, names):
        """first[k] = the smallest LOCAL record index whose name equals names[k] (a list of bytes, or (uint8 chars, uint64
        offsets)), _abi.NAME_NOT_FOUND where no record has it: find_names' answer, from the table names_build left on the device
        (crass_hip_fastx_names_find).  Returns uint64 [n]."""
        chars, off = _names_arg(names)
        m = max(len(off) - 1, 0)
        out = np.zeros(m, np.uint64)
        _chk(self.lib.crass_hip_fastx_names_find(self.h, chars.ctypes.data if len(chars) else None, off.ctypes.data if len(off) else None, m,
                                                 out.ctypes.data if m else None), "crass_hip_fastx_names_find")
        return out

    def _names_out(self, st, where, n, d_off, total):
        if st != 0:
            e = CrassError(st, where)
            e.n, e.total = int(n), int(total)
            raise e
        return int(n), int(total)

    def names_of_device(self, idx, out_chars, out_off, idx_base=0):
        """The NAMES of the records idx[k] - idx_base of the table names_build keeps, back to back in out_chars with their offsets
        (n + 1) in out_off, everything in DEVICE memory (crass_hip_fastx_names_of_device): idx and out_off are contiguous torch
        int64 device tensors or (address, elements), out_chars a torch uint8 device tensor or (address, bytes).  Returns the
        total bytes, the call's one host read.  An out_chars too small raises CrassError with status 8, `total` set, the offsets
        complete and nothing written at or beyond its end."""
        pi, n = _device_array(idx, "int64", "names_of_device(idx)")
        pc, cap = _device_array(out_chars, "uint8", "names_of_device(out_chars)")
        po, no = _device_array(out_off, "int64", "names_of_device(out_off)")
        if no < n + 1:
            raise ValueError("names_of_device(out_off) needs n + 1 elements")
        total = C.c_uint64()
        st = self.lib.crass_hip_fastx_names_of_device(self.h, pi, n, int(idx_base), pc, cap, po, C.byref(total))
        return self._names_out(st, "crass_hip_fastx_names_of_device", n, po, total.value)[1]

    def found_names_device(self, out_chars, out_off):
        """The NAMES of this context's pass-1 records, in record order, into DEVICE memory (crass_hip_found_names_device): what a
        rank publishes for the found headers of other ranks, without the caller holding the records' indices.  out_chars /
        out_off as names_of_device takes them (out_off: room for cap_names + 1 offsets).  Returns (n, total); too small a
        buffer raises CrassError with status 8 and `n` / `total` set."""
        pc, cap = _device_array(out_chars, "uint8", "found_names_device(out_chars)")
        po, no = _device_array(out_off, "int64", "found_names_device(out_off)")
        n, total = C.c_uint64(), C.c_uint64()
        st = self.lib.crass_hip_found_names_device(self.h, pc, cap, po, max(no - 1, 0), C.byref(n), C.byref(total))
        return self._names_out(st, "crass_hip_found_names_device", n.value, po, total.value)

    def names_find_device(self, names, name_off, out_first, n_name_bytes=None):
        """names_find with the queries (names: uint8, name_off: int64 [n + 1]) and the answers (out_first: int64 [n]; an answer's
        bits are the uint64 of names_find, -1 where no record has the name) in DEVICE memory: torch device tensors or (address,
        elements) (crass_hip_fastx_names_find_device).  n_name_bytes: the bytes of names the offsets may refer to (default: all
        of the tensor)."""
        pn, nb = _device_array(names, "uint8", "names_find_device(names)")
        po, no = _device_array(name_off, "int64", "names_find_device(name_off)")
        pf, nf = _device_array(out_first, "int64", "names_find_device(out_first)")
        m = max(no - 1, 0)
        if nf < m:
            raise ValueError("names_find_device(out_first) needs one element per query")
        _chk(self.lib.crass_hip_fastx_names_find_device(self.h, pn, nb if n_name_bytes is None else int(n_name_bytes), po, m, pf),
             "crass_hip_fastx_names_find_device")

    def names_drop(self):
        """Gives the table of names_build back (crass_hip_fastx_names_drop); fine without one."""
        _chk(self.lib.crass_hip_fastx_names_drop(self.h), "crass_hip_fastx_names_drop")
        self._names_keep = None

    def last_names_ms(self):
        """HIP-event milliseconds of (the last names_build's insert launches, the last names_find's kernels); stage timing >= 1,
        else zeros."""
        return tuple(float(self.lib.crass_hip_last_names_ms(self.h, k)) for k in range(2))

    def fetch_header_lines(self, src, layout, idx, out=None):
        """The header lines (without the header character and the line end) of the records idx (LOCAL record numbers, any order,
        repeats allowed) of file bytes on the DEVICE (crass_hip_fetch_header_lines_device).  Returns (chars, off, name_len):
        numpy copies of the lines back to back (uint8), their offsets (uint64, n + 1) and the length of the name at each line's
        start (uint32).  out: a contiguous torch uint8 DEVICE tensor — the lines are written there instead
        (crass_hip_fetch_header_lines_device_to) and chars is None; a tensor too small raises CrassError with status 8 and the
        offsets in its `offsets`."""
        ptr, nb, rp, n = self._device_bytes(src, layout)
        a = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
        name_len = np.zeros(len(a), np.uint32)
        args = (self.h, ptr, nb, rp.ctypes.data if n else None, n, a.ctypes.data if len(a) else None, len(a))
        if out is None:
            v = _abi.Text()
            _chk(self.lib.crass_hip_fetch_header_lines_device(*args, C.byref(v), name_len.ctypes.data if len(a) else None),
                 "crass_hip_fetch_header_lines_device")
            t = Text(v)
            return t.chars.copy(), t.off.copy(), name_len
        if str(out.dtype) != "torch.uint8" or not out.is_cuda or not out.is_contiguous():
            raise ValueError("fetch_header_lines(out=...) needs a contiguous uint8 device tensor")
        off = np.zeros(len(a) + 1, np.uint64)
        st = self.lib.crass_hip_fetch_header_lines_device_to(*args, int(out.data_ptr()) if out.numel() else None, int(out.numel()), off.ctypes.data,
                                                             name_len.ctypes.data if len(a) else None)
        if st != 0:
            e = CrassError(st, "crass_hip_fetch_header_lines_device_to")
            e.offsets = off
            raise e
        return None, off, name_len

    def comments_build(self, src=None, layout=None, file_read_base=None):
        """Builds and KEEPS the own-comment bitmap and tile carries of file bytes on the DEVICE (src, layout: as
        fetch_header_lines takes them; file_read_base: n_files + 1 read bases, None: one file) for fetch_comments
        (crass_hip_fastx_comments_build_device).  The structure refers to the bytes: keep the tensor alive and unchanged until
        comments_drop, the next comments_build, any load, or close.  comments_build(): the arena and layout of the last
        load_fastx_files (fetch_comments does this by itself)."""
        if src is None and layout is None:
            _chk(self.lib.crass_hip_fastx_comments_build_device(self.h, None, 0, None, 0, None, 0), "crass_hip_fastx_comments_build_device")
            self._comments_keep = None
            return
        ptr, nb, rp, n = self._device_bytes(src, layout)
        fb = None if file_read_base is None else np.ascontiguousarray(file_read_base, dtype=np.uint64)
        _chk(self.lib.crass_hip_fastx_comments_build_device(self.h, ptr, nb, rp.ctypes.data, n, None if fb is None else fb.ctypes.data,
                                                            0 if fb is None else len(fb) - 1), "crass_hip_fastx_comments_build_device")
        self._comments_keep = src

    def comments_drop(self):
        """Gives the structure of comments_build back (crass_hip_fastx_comments_drop); fine without one."""
        _chk(self.lib.crass_hip_fastx_comments_drop(self.h), "crass_hip_fastx_comments_drop")
        self._comments_keep = None

    def comments_counters(self):
        """(records with a comment of their own, records) of the built structure (crass_hip_fastx_comments_counters)."""
        out = (C.c_uint64 * 2)()
        _chk(self.lib.crass_hip_fastx_comments_counters(self.h, C.byref(out)), "crass_hip_fastx_comments_counters")
        return int(out[0]), int(out[1])

    def last_comments_ms(self):
        """HIP-event milliseconds of (the last comments_build's launches, the last fetch_comments' kernels); stage timing >= 1,
        else zeros."""
        return tuple(float(self.lib.crass_hip_last_comments_ms(self.h, k)) for k in range(2))

    def fetch_comments(self, idx, out=None):
        """The comment kseq HANDS to the records idx (LOCAL record numbers, any order, repeats allowed), from the structure
        comments_build keeps — after load_fastx_files the first call builds it on the arena (crass_hip_fetch_comments_device).
        Returns (chars, off, has): numpy copies of the comments back to back (uint8), their offsets (uint64, n + 1) and whether
        a comment is handed at all (uint8; it may be empty).  out: a contiguous torch uint8 DEVICE tensor — the comments are
        written there instead (crass_hip_fetch_comments_device_to) and chars is None; a tensor too small raises CrassError with
        status 8 and the offsets / has in its `offsets` / `has`."""
        a = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
        has = np.zeros(len(a), np.uint8)
        args = (self.h, a.ctypes.data if len(a) else None, len(a))
        if out is None:
            v = _abi.Text()
            _chk(self.lib.crass_hip_fetch_comments_device(*args, C.byref(v), has.ctypes.data if len(a) else None), "crass_hip_fetch_comments_device")
            t = Text(v)
            return t.chars.copy(), t.off.copy(), has
        if str(out.dtype) != "torch.uint8" or not out.is_cuda or not out.is_contiguous():
            raise ValueError("fetch_comments(out=...) needs a contiguous uint8 device tensor")
        off = np.zeros(len(a) + 1, np.uint64)
        st = self.lib.crass_hip_fetch_comments_device_to(*args, int(out.data_ptr()) if out.numel() else None, int(out.numel()), off.ctypes.data,
                                                         has.ctypes.data if len(a) else None)
        if st != 0:
            e = CrassError(st, "crass_hip_fetch_comments_device_to")
            e.offsets, e.has = off, has
            raise e
        return None, off, has

    def last_scan_ms(self):
        """HIP-event milliseconds of the last load_fastx_bytes / attach_device_fastx call's scan kernels (stage timing >= 1, else 0)."""
        return float(self.lib.crass_hip_last_scan_ms(self.h))

    def fetch_text(self, idx, revcomp=None, out=None):
        """The text of the reads idx (GLOBAL indices: candidates' / recruits' read_idx as they are), reverse-complemented
        where revcomp[k] is set, unpacked on the device (crass_hip_fetch_text).  Returns a Text.  out: a contiguous torch
        uint8 DEVICE tensor — the text is written there instead (crass_hip_fetch_text_device) and the offsets (uint64,
        n + 1) are returned; a tensor too small raises CrassError with status 8 and the offsets in its `offsets`."""
        a, rc = _fetch_args(idx, revcomp)
        if out is None:
            v = _abi.Text()
            _chk(self.lib.crass_hip_fetch_text(self.h, a.ctypes.data if len(a) else None, None if rc is None else rc.ctypes.data, len(a),
                                               C.byref(v)), "crass_hip_fetch_text")
            return Text(v)
        if str(out.dtype) != "torch.uint8" or not out.is_cuda or not out.is_contiguous():
            raise ValueError("fetch_text(out=...) needs a contiguous uint8 device tensor")
        off = np.zeros(len(a) + 1, np.uint64)
        st = self.lib.crass_hip_fetch_text_device(self.h, a.ctypes.data if len(a) else None, None if rc is None else rc.ctypes.data, len(a),
                                                  int(out.data_ptr()) if out.numel() else None, int(out.numel()), off.ctypes.data)
        if st != 0:
            e = CrassError(st, "crass_hip_fetch_text_device")
            e.offsets = off
            raise e
        return off

    def fetch_record_text(self, pass_):
        """RH_Seq of every record of the last pass 1 (pass_ = 1: the candidates' order) or pass 2 (2: the recruits'): the
        read's text, reverse-complemented where low_lexi is 0 (crass_hip_fetch_record_text).  Returns a Text."""
        v = _abi.Text()
        _chk(self.lib.crass_hip_fetch_record_text(self.h, int(pass_), C.byref(v)), "crass_hip_fetch_record_text")
        return Text(v)

    def last_fetch_ms(self):
        """HIP-event milliseconds of the last fetch's kernel (stage timing >= 1, else 0)."""
        return float(self.lib.crass_hip_last_fetch_ms(self.h))

    def packed(self):
        """The resident read set copied back (crass_hip_get_packed): a ResidentReads with PackedReads' fields."""
        return ResidentReads(self)

    # ---- passes ----
    def seed_scan(self, fetch=True):
        _chk(self.lib.crass_hip_seed_scan(self.h), "crass_hip_seed_scan")
        return self.candidates() if fetch else None

    def candidates(self):
        v = _abi.Candidates()
        _chk(self.lib.crass_hip_get_candidates(self.h, C.byref(v)), "crass_hip_get_candidates")
        return CandidateSet(v)

    def candidate_dr_view(self):
        """(uint8 array [n, dr_stride], uint16 lengths) without copying the other fields."""
        v = _abi.Candidates()
        _chk(self.lib.crass_hip_get_candidates(self.h, C.byref(v)), "crass_hip_get_candidates")
        n = int(v.n)
        chars = _np(C.cast(v.dr_chars, _abi.u8p), n * int(v.dr_stride), np.uint8).reshape(n, int(v.dr_stride))
        return chars, _np(v.dr_len, n, np.uint16)

    def merge(self, dr_chars=None, dr_len=None, fetch=True):
        """dr_chars: uint8 array [n, stride] of ALL candidates in global read order (multi-GPU),
        or None for this context's own candidates."""
        if dr_chars is None:
            _chk(self.lib.crass_hip_merge(self.h, None, None, 0, 0), "crass_hip_merge")
        else:
            dr_chars = np.ascontiguousarray(dr_chars, dtype=np.uint8)
            dr_len = np.ascontiguousarray(dr_len, dtype=np.uint16)
            n = dr_chars.shape[0]
            stride = dr_chars.shape[1] if n else 16
            _chk(self.lib.crass_hip_merge(self.h, dr_chars.ctypes.data, dr_len.ctypes.data, int(stride), int(n)),
                 "crass_hip_merge")
        return self.merge_view() if fetch else None

    def distinct(self):
        """(uint8 [n_distinct, stride], uint16 [n_distinct], uint32 cand->distinct map) of this
        context's pass-1 candidates, first-occurrence order (the compact multi-GPU payload)."""
        v = _abi.Distinct()
        _chk(self.lib.crass_hip_get_distinct(self.h, C.byref(v)), "crass_hip_get_distinct")
        nd, st = int(v.n_distinct), int(v.dr_stride)
        chars = _np(C.cast(v.dr_chars, _abi.u8p), nd * st, np.uint8).reshape(nd, st)
        return chars, _np(v.dr_len, nd, np.uint16), _np(v.cand_distinct, int(v.n_candidates), np.uint32)

    def merge_distinct(self, g_chars, g_lens, my_offset, fetch=True):
        """merge from the rank-ordered concatenation of every rank's distinct list"""
        g_chars = np.ascontiguousarray(g_chars, dtype=np.uint8)
        g_lens = np.ascontiguousarray(g_lens, dtype=np.uint16)
        n = g_chars.shape[0]
        stride = g_chars.shape[1] if n else 16
        _chk(self.lib.crass_hip_merge_distinct(self.h, g_chars.ctypes.data, g_lens.ctypes.data, int(stride), int(n),
                                               int(my_offset)), "crass_hip_merge_distinct")
        return self.merge_view() if fetch else None

    def distinct_device(self):
        """(device pointer of the distinct strings, device pointer of their lengths, n, stride) or None when
        pass 1 did not leave the list on the device"""
        v = _abi.DistinctDev()
        st = self.lib.crass_hip_get_distinct_device(self.h, C.byref(v))
        if st != 0:
            return None
        return int(v.d_chars or 0), int(v.d_len or 0), int(v.n_distinct), int(v.dr_stride)

    def merge_distinct_device(self, d_chars_ptr, d_len_ptr, stride, n_global, my_offset, fetch=True):
        """merge from a DEVICE-resident rank-ordered concatenation of every rank's distinct list"""
        _chk(self.lib.crass_hip_merge_distinct_device(self.h, C.c_void_p(d_chars_ptr), C.c_void_p(d_len_ptr), int(stride), int(n_global),
                                                      int(my_offset)), "crass_hip_merge_distinct_device")
        return self.merge_view() if fetch else None

    def exchange_setup(self, world, rank, cap_rows):
        """one-collective exchange: returns (device pointer of the send buffer, its size in bytes)"""
        x = _abi.Exchange()
        _chk(self.lib.crass_hip_exchange_setup(self.h, int(world), int(rank), int(cap_rows), C.byref(x)), "crass_hip_exchange_setup")
        return int(x.d_send), int(x.send_bytes)

    def exchange_set_deferred(self, on=True):
        """seed_scan() returns with pass 1 still queued; the collective goes on the engine's stream (crass_hip_exchange_set_deferred)"""
        _chk(self.lib.crass_hip_exchange_set_deferred(self.h, 1 if on else 0), "crass_hip_exchange_set_deferred")

    def merge_gathered(self, d_recv_ptr, fetch=True):
        """merge from the all-gathered send buffers (device pointer).  Returns None, or the number of rows the
        exchange needs when some rank's list did not fit (set up again, repeat seed scan + collective)."""
        st = self.lib.crass_hip_merge_gathered(self.h, C.c_void_p(d_recv_ptr))
        if st == _abi.ERR_OVERFLOW:
            return int(self.lib.crass_hip_exchange_needed_rows(self.h))
        _chk(st, "crass_hip_merge_gathered")
        return self.merge_view() if fetch else None

    def merge_view(self):
        v = _abi.MergeView()
        _chk(self.lib.crass_hip_get_merge(self.h, C.byref(v)), "crass_hip_get_merge")
        return MergeResult(v)

    def set_patterns(self, patterns):
        arr = (C.c_char_p * len(patterns))(*patterns)
        lens = (C.c_uint32 * len(patterns))(*[len(p) for p in patterns])
        _chk(self.lib.crass_hip_set_patterns(self.h, arr, lens, len(patterns)), "crass_hip_set_patterns")

    def recruit(self, extra_found=None, fetch=True, extra_found_device=None):
        """extra_found_device: a second list of found reads in DEVICE memory (a contiguous torch int64 device tensor or (address,
        elements)) that may hold -1, names_find_device's "no record" (crass_hip_recruit_found)."""
        ef = None
        if extra_found is not None and len(extra_found):
            ef = np.ascontiguousarray(extra_found, dtype=np.uint64)
        if extra_found_device is not None:
            pd, nd = _device_array(extra_found_device, "int64", "recruit(extra_found_device)")
            _chk(self.lib.crass_hip_recruit_found(self.h, None if ef is None else ef.ctypes.data, 0 if ef is None else len(ef), pd, nd),
                 "crass_hip_recruit_found")
        elif ef is not None:
            _chk(self.lib.crass_hip_recruit(self.h, ef.ctypes.data, len(ef)), "crass_hip_recruit")
        else:
            _chk(self.lib.crass_hip_recruit(self.h, None, 0), "crass_hip_recruit")
        return self.recruits() if fetch else None

    def recruits(self):
        v = _abi.Recruits()
        _chk(self.lib.crass_hip_get_recruits(self.h, C.byref(v)), "crass_hip_get_recruits")
        return RecruitSet(v)

    def fetch_abi(self):
        """the three getters of the ABI (crass_hip_get_candidates / _get_merge / _get_recruits) and nothing else: what an adapter
        pays on top of a step to see the wide per-record arrays (the step itself ends with compact blobs in pinned memory).
        Returns (n_candidates, n_tokens, n_recruits)."""
        c, m, q = _abi.Candidates(), _abi.MergeView(), _abi.Recruits()
        _chk(self.lib.crass_hip_get_candidates(self.h, C.byref(c)), "crass_hip_get_candidates")
        _chk(self.lib.crass_hip_get_merge(self.h, C.byref(m)), "crass_hip_get_merge")
        _chk(self.lib.crass_hip_get_recruits(self.h, C.byref(q)), "crass_hip_get_recruits")
        return int(c.n), int(m.n_tokens), int(q.n)

    def stream_wait_event(self, event_handle):
        """order the engine's stream behind a HIP event (raw hipEvent_t handle, e.g. torch.cuda.Event().cuda_event)"""
        _chk(self.lib.crass_hip_stream_wait_event(self.h, C.c_void_p(int(event_handle))), "crass_hip_stream_wait_event")

    def set_host_view(self, light):
        """1: after a device merge this context only builds its own candidates' tokens (ranks other than 0 of a multi-rank job:
        tokens, groups and patterns are identical on every rank); 0: the full host view (crass_hip_set_host_view)"""
        _chk(self.lib.crass_hip_set_host_view(self.h, 1 if light else 0), "crass_hip_set_host_view")

    def set_timing_focus(self, kernels):
        """level 1: bit 0 seed scan, bit 1 survivors, bit 2 pass-2 scan (crass_hip_set_timing_focus)"""
        _chk(self.lib.crass_hip_set_timing_focus(self.h, int(kernels)), "crass_hip_set_timing_focus")

    def set_stage_timing(self, level):
        """0 none (default), 1 the three large kernels, 2 every stage — see crass_hip_set_stage_timing."""
        _chk(self.lib.crass_hip_set_stage_timing(self.h, int(level)), "crass_hip_set_stage_timing")

    def reload_env(self):
        """re-read the environment's A/B and test switches (they are read once, at creation)"""
        _chk(self.lib.crass_hip_reload_env(self.h), "crass_hip_reload_env")

    def counters(self):
        c = _abi.Counters()
        _chk(self.lib.crass_hip_get_counters(self.h, C.byref(c)), "crass_hip_get_counters")
        return c.asdict()

    def stream_handle(self):
        return self.lib.crass_hip_stream(self.h)

    def levenshtein_batch(self, pairs, want_similarity=True):
        """pairs: list of (bytes, bytes) -> (int32 distances, float32 similarities)"""
        items = []
        a_off, a_len, b_off, b_len = [], [], [], []
        pos = 0
        for a, b in pairs:
            a_off.append(pos); a_len.append(len(a)); items.append(a); pos += len(a)
            b_off.append(pos); b_len.append(len(b)); items.append(b); pos += len(b)
        chars = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8).copy()
        a_off = np.array(a_off, np.uint64); b_off = np.array(b_off, np.uint64)
        a_len = np.array(a_len, np.uint32); b_len = np.array(b_len, np.uint32)
        dist = np.zeros(len(pairs), np.int32)
        sim = np.zeros(len(pairs), np.float32)
        _chk(self.lib.crass_hip_levenshtein_batch(self.h, chars.ctypes.data, pos, a_off.ctypes.data, a_len.ctypes.data,
                                                  b_off.ctypes.data, b_len.ctypes.data, len(pairs), dist.ctypes.data,
                                                  sim.ctypes.data if want_similarity else None),
             "crass_hip_levenshtein_batch")
        return dist, sim


class SearchGroup:
    """Several GPUs from one process (crass_hip_group_*): contiguous read shards, one RCCL all-gather of the distinct
    candidate DR strings per step issued by the engine, one host view for the group.  devices: list of device
    indices; local_copies=True replaces the collective by device copies (tests: several contexts on one GPU)."""

    GROUP_LOCAL_COPIES = 1

    def __init__(self, devices, params=None, local_copies=False):
        self.lib = _abi.load()
        self.params = params or default_params()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        st = self.lib.crass_hip_group_create(C.byref(self.params), devs, len(devices), self.GROUP_LOCAL_COPIES if local_copies else 0,
                                             C.byref(h))
        if st != 0:
            raise CrassError(st, "crass_hip_group_create [%s]" % self.lib.crass_hip_group_last_error().decode())
        self.h = h
        self.n = len(devices)
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.crass_hip_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, st, where):
        if st != 0:
            raise CrassError(st, "%s [%s]" % (where, self.lib.crass_hip_group_last_error().decode()))

    @property
    def rccl_ranks(self):
        return int(self.lib.crass_hip_group_rccl_ranks(self.h))

    def load_reads(self, packed, header_id=None, read_index_base=0):
        r = _abi.Reads()
        C.memmove(C.byref(r), C.byref(packed.reads), C.sizeof(r))
        hid = None
        if header_id is not None:
            hid = np.ascontiguousarray(header_id, dtype=np.uint64)
            r.header_id = hid.ctypes.data
        r.read_index_base = int(read_index_base)
        self._chk(self.lib.crass_hip_group_load_reads(self.h, C.byref(r)), "crass_hip_group_load_reads")

    def load_packed_uniform(self, words, n_reads, read_len, read_index_base=0):
        r = _abi.Reads()
        r.n_reads = int(n_reads)
        r.packed = words.ctypes.data
        r.stride_words = (int(read_len) + 15) // 16
        r.uniform_len = int(read_len)
        r.read_index_base = int(read_index_base)
        self._chk(self.lib.crass_hip_group_load_reads(self.h, C.byref(r)), "crass_hip_group_load_reads")

    def seed_scan(self):
        self._chk(self.lib.crass_hip_group_seed_scan(self.h), "crass_hip_group_seed_scan")

    def merge(self):
        self._chk(self.lib.crass_hip_group_merge(self.h), "crass_hip_group_merge")

    def recruit(self, extra_found=None):
        if extra_found is not None and len(extra_found):
            ef = np.ascontiguousarray(extra_found, dtype=np.uint64)
            self._chk(self.lib.crass_hip_group_recruit(self.h, ef.ctypes.data, len(ef)), "crass_hip_group_recruit")
        else:
            self._chk(self.lib.crass_hip_group_recruit(self.h, None, 0), "crass_hip_group_recruit")

    def set_patterns(self, patterns):
        arr = (C.c_char_p * len(patterns))(*patterns)
        lens = (C.c_uint32 * len(patterns))(*[len(p) for p in patterns])
        self._chk(self.lib.crass_hip_group_set_patterns(self.h, arr, lens, len(patterns)), "crass_hip_group_set_patterns")

    def step(self):
        self._chk(self.lib.crass_hip_group_step(self.h), "crass_hip_group_step")

    def candidates(self):
        v = _abi.Candidates()
        self._chk(self.lib.crass_hip_group_get_candidates(self.h, C.byref(v)), "crass_hip_group_get_candidates")
        return CandidateSet(v)

    def merge_view(self):
        v = _abi.MergeView()
        self._chk(self.lib.crass_hip_group_get_merge(self.h, C.byref(v)), "crass_hip_group_get_merge")
        return MergeResult(v)

    def recruits(self):
        v = _abi.Recruits()
        self._chk(self.lib.crass_hip_group_get_recruits(self.h, C.byref(v)), "crass_hip_group_get_recruits")
        return RecruitSet(v)

    def fetch_text(self, idx, revcomp=None):
        """SearchEngine.fetch_text over the whole job: every global index goes to the rank whose shard holds it, the records
        come back in idx's order (crass_hip_group_fetch_text).  Returns a Text owned by the group."""
        a, rc = _fetch_args(idx, revcomp)
        v = _abi.Text()
        self._chk(self.lib.crass_hip_group_fetch_text(self.h, a.ctypes.data if len(a) else None, None if rc is None else rc.ctypes.data,
                                                      len(a), C.byref(v)), "crass_hip_group_fetch_text")
        return Text(v)

    def load_fastx_files(self, files, pad_uniform=2, nominal=None):
        """Several input files' bytes (plain FASTA / FASTQ or BGZF) cut into record-aligned shards, one per rank, each parsed on
        its rank's device beside the others (crass_hip_group_load_fastx_files).  nominal: n - 1 non-decreasing positions in the
        job's text space (None: even cuts).  Returns a FastxShards; raises FastxFilesDeclined (status 2, no rank holds reads)
        when a file is declined, with the shards' decline fields in its `layout`."""
        arrs, ptrs, lens = _files_args(files)
        nom = _nominal_arg(nominal, self.n)
        v = _abi.FastxShardsC()
        st = self.lib.crass_hip_group_load_fastx_files(self.h, ptrs, lens.ctypes.data_as(_abi.u64p), len(arrs), int(pad_uniform),
                                                       nom.ctypes.data if nom is not None and len(nom) else None, C.byref(v))
        sh = FastxShards(v)
        if st == 2 and not sh.accepted:
            raise FastxFilesDeclined(st, "crass_hip_group_load_fastx_files", sh)
        self._chk(st, "crass_hip_group_load_fastx_files")
        return sh

    def fetch_comments(self, idx):
        """The comment kseq HANDS to reads of the whole job (global indices) of a group loaded by load_fastx_files
        (crass_hip_group_fetch_comments): carried across the ranks' cuts inside a file, never across a file boundary.  Returns
        (chars, off, has) as SearchEngine.fetch_comments."""
        a = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
        has = np.zeros(len(a), np.uint8)
        v = _abi.Text()
        self._chk(self.lib.crass_hip_group_fetch_comments(self.h, a.ctypes.data if len(a) else None, len(a), C.byref(v),
                                                          has.ctypes.data if len(a) else None), "crass_hip_group_fetch_comments")
        t = Text(v)
        return t.chars.copy(), t.off.copy(), has

    def fetch_header_lines(self, idx):
        """The header lines of the reads idx (GLOBAL read indices, any order) of the last load_fastx_files, from the ranks' arenas
        (crass_hip_group_fetch_header_lines).  Returns (chars, off, name_len): numpy copies of the lines back to back, their
        offsets (n + 1) and the length of the NAME at each line's start."""
        a = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
        nl = np.zeros(len(a), np.uint32)
        v = _abi.Text()
        self._chk(self.lib.crass_hip_group_fetch_header_lines(self.h, a.ctypes.data if len(a) else None, len(a), C.byref(v),
                                                              nl.ctypes.data if len(a) else None), "crass_hip_group_fetch_header_lines")
        t = Text(v)
        return t.chars.copy(), t.off.copy(), nl

    def fetch_quality(self, idx):
        """The quality strings of the reads idx (GLOBAL read indices) of the last load_fastx_files
        (crass_hip_group_fetch_quality).  Returns (chars, off, has_qual) as SearchEngine.fetch_quality."""
        a = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64).reshape(-1))
        has = np.zeros(len(a), np.uint8)
        v = _abi.Text()
        self._chk(self.lib.crass_hip_group_fetch_quality(self.h, a.ctypes.data if len(a) else None, len(a), C.byref(v),
                                                         has.ctypes.data if len(a) else None), "crass_hip_group_fetch_quality")
        t = Text(v)
        return t.chars.copy(), t.off.copy(), has

    def set_fastq_class(self, fastq_class):
        """The class load_fastx_files reads FASTQ by (crass_hip_group_set_fastq_class; CRASS_DEVICE_FASTQ=wrapped at creation does
        the same): 0, the default, the four-line form only; 1 also records over several lines and blank lines — a load that the
        four-line cut declines for a FASTQ's shape runs once more with every FASTQ file cut at the records reachable from its
        line 0.  Also set on every rank's context, so fetch_quality reads by the wrapped rule."""
        self._chk(self.lib.crass_hip_group_set_fastq_class(self.h, int(fastq_class)), "crass_hip_group_set_fastq_class")

    def inflate_gzip(self, buf, chunk_bytes=0, nominal=None, out_cap=None, with_plan=False):
        """The text of a plain (single-member) gzip file's bytes, inflated across the ranks (crass_hip_group_inflate_gzip): chunks
        dealt over the ranks for find and count, every rank the elements of its range of the text (nominal: size - 1 text
        positions; None: even) with symbolic windows, the entry windows composed on the host.  Host memory in, host memory out;
        results and errors as gzip_inflate_ranges_host with n_ranges = the group's size."""
        a = _bytes_arg(buf)
        nom = _nominal_arg(nominal, self.n)
        ptr = a.ctypes.data if len(a) else None
        return _gzip_ranges_call("crass_hip_group_inflate_gzip", lambda o, cap, n, p, v: self.lib.crass_hip_group_inflate_gzip(
            self.h, ptr, len(a), int(chunk_bytes), nom.ctypes.data if nom is not None and len(nom) else None, o, cap, n, p, v), a, out_cap, with_plan)

    def inflate_gzip_members(self, buf, chunk_bytes=0, nominal=None, out_cap=None, with_plan=False):
        """inflate_gzip for a plain gzip file of any number of members (crass_hip_group_inflate_gzip_members): the members rule by
        ranges.  Results and errors as gzip_inflate_members_ranges_host with n_ranges = the group's size; with with_plan
        (text, GzipPlan, GzipMembers)."""
        a = _bytes_arg(buf)
        nom = _nominal_arg(nominal, self.n)
        ptr = a.ctypes.data if len(a) else None
        return _gzip_members_ranges_call("crass_hip_group_inflate_gzip_members", lambda o, cap, n, p, m, v: self.lib.crass_hip_group_inflate_gzip_members(
            self.h, ptr, len(a), int(chunk_bytes), nom.ctypes.data if nom is not None and len(nom) else None, o, cap, n, p, m, v), a, out_cap,
            with_plan)

    def gzip_members_counters(self):
        """(files taken in members mode, their members, CRC pieces summed over the ranks, exported windows that held no reference)
        of the last inflate_gzip_members, or summed over the files the last load_fastx_files took in members mode
        (crass_hip_group_gzip_members_counters)."""
        out = np.zeros(4, np.uint64)
        self._chk(self.lib.crass_hip_group_gzip_members_counters(self.h, out.ctypes.data), "crass_hip_group_gzip_members_counters")
        return tuple(int(x) for x in out)

    def gzip_members_ms(self, rank):
        """HIP-event milliseconds of a rank's k_gz_member_crc in the last inflate_gzip_members, or for the last gzip file of the
        last load_fastx_files in members mode (crass_hip_group_gzip_members_ms): a dict of member_crc; measured at stage timing
        level >= 1.  gzip_ms's narrow does not hold it."""
        out = np.zeros(1, np.float32)
        self._chk(self.lib.crass_hip_group_gzip_members_ms(self.h, int(rank), out.ctypes.data), "crass_hip_group_gzip_members_ms")
        return {"member_crc": float(out[0])}

    def set_gzip_on_device(self, mode, chunk_bytes=0):
        """load_fastx_files takes plain gzip files (crass_hip_group_set_gzip_on_device): 0 / False, the default,
        declines them as before; 2 takes plain gzip of any number of members; anything else single-member files only (further
        members: 13).  Such a file is taken as a BGZF file is taken, chain elements for members: an index step
        (find, count, the chain) before the shards are cut, then every rank inflates the elements of its pieces and keeps their text
        on its device; tails and wrapped-mode margins pull further elements through a seeded window walk.  chunk_bytes: 0 the
        default chunk."""
        self._chk(self.lib.crass_hip_group_set_gzip_on_device(self.h, int(mode), int(chunk_bytes)), "crass_hip_group_set_gzip_on_device")

    def gzip_counters(self):
        """(gzip files taken, chunks, chain elements, elements inflated by a further rank, compressed bytes uploaded, of them
        uploaded before) of the last inflate_gzip, or summed over the gzip files the last load_fastx_files took — the elements its
        seeded walks added count as inflated by a further rank (crass_hip_group_gzip_counters)."""
        out = np.zeros(6, np.uint64)
        self._chk(self.lib.crass_hip_group_gzip_counters(self.h, out.ctypes.data), "crass_hip_group_gzip_counters")
        return tuple(int(x) for x in out)

    def gzip_ms(self, rank):
        """HIP-event milliseconds of a rank's kernels in the last inflate_gzip, or for the last gzip file of the last
        load_fastx_files (crass_hip_group_gzip_ms): a dict of find, count, decode, windows_sym, resolve, narrow, and tail_windows:
        the seeded window walks of the last load_fastx_files, summed (0 after inflate_gzip); measured at stage timing level >= 1."""
        out = np.zeros(7, np.float32)
        self._chk(self.lib.crass_hip_group_gzip_ms(self.h, int(rank), out.ctypes.data), "crass_hip_group_gzip_ms")
        return dict(zip(("find", "count", "decode", "windows_sym", "resolve", "narrow", "tail_windows"), (float(x) for x in out)))

    def load_counters(self):
        """(attempts, files cut by the wrapped rule, margin doublings, chain look-ups) of the last load_fastx_files
        (crass_hip_group_load_counters)."""
        out = np.zeros(4, np.uint64)
        self._chk(self.lib.crass_hip_group_load_counters(self.h, out.ctypes.data), "crass_hip_group_load_counters")
        return tuple(int(x) for x in out)

    def set_name_exchange(self, on_device):
        """The route of the found-name exchange of a files load: False the host's (the default), True everything in device memory
        (crass_hip_group_set_name_exchange; CRASS_GROUP_NAMES=device at creation does the same)."""
        self._chk(self.lib.crass_hip_group_set_name_exchange(self.h, 1 if on_device else 0), "crass_hip_group_set_name_exchange")

    def name_exchange_counters(self, rank):
        """(route of the last step's exchange: 0 host / 1 device, names published, queries looked up, namesakes found) of a rank
        (crass_hip_group_name_exchange_counters)."""
        out = np.zeros(4, np.uint64)
        self._chk(self.lib.crass_hip_group_name_exchange_counters(self.h, int(rank), out.ctypes.data), "crass_hip_group_name_exchange_counters")
        return tuple(int(x) for x in out)

    def name_exchange_ms(self, rank):
        """(wall ms, HIP-event ms) of the last step's exchange on a rank, publish to lookup (crass_hip_group_name_exchange_ms); the
        event time only in a group created with CRASS_GROUP_NAMES_TIMING set, else 0."""
        out = np.zeros(2, np.float32)
        self._chk(self.lib.crass_hip_group_name_exchange_ms(self.h, int(rank), out.ctypes.data), "crass_hip_group_name_exchange_ms")
        return float(out[0]), float(out[1])

    def rank_counters(self, rank):
        c = _abi.Counters()
        _chk(self.lib.crass_hip_get_counters(C.c_void_p(self.lib.crass_hip_group_ctx(self.h, int(rank))), C.byref(c)), "crass_hip_get_counters")
        return c.asdict()

    def rank_last_scan_classes(self, rank):
        """(pieces the four-line scan decided, pieces the wrapped scan decided) of a rank's last load (crass_hip_last_scan_classes)"""
        out = (C.c_uint64 * 2)()
        _chk(self.lib.crass_hip_last_scan_classes(C.c_void_p(self.lib.crass_hip_group_ctx(self.h, int(rank))), out), "crass_hip_last_scan_classes")
        return int(out[0]), int(out[1])

    def rank_last_cut_chain_ms(self, rank):
        """HIP-event ms of a rank's cut kernels in the last wrapped-mode load_fastx_files (crass_hip_last_cut_chain_ms; stage timing >= 1)"""
        return float(self.lib.crass_hip_last_cut_chain_ms(C.c_void_p(self.lib.crass_hip_group_ctx(self.h, int(rank)))))

    def rank_set_stage_timing(self, rank, level):
        _chk(self.lib.crass_hip_set_stage_timing(C.c_void_p(self.lib.crass_hip_group_ctx(self.h, int(rank))), int(level)), "crass_hip_set_stage_timing")

    def rank_set_timing_focus(self, rank, kernels):
        _chk(self.lib.crass_hip_set_timing_focus(C.c_void_p(self.lib.crass_hip_group_ctx(self.h, int(rank))), int(kernels)), "crass_hip_set_timing_focus")

    def result(self):
        """the whole job's hand-off as a PipelineResult (same fields as search_pipeline's)"""
        cand, merge, rec = self.candidates(), self.merge_view(), self.recruits()
        res = PipelineResult(cand, merge, rec, cand.max_read_len)
        res.counters = [self.rank_counters(r) for r in range(self.n)]
        return res


def search_pipeline_group(seqs, devices, headers=None, params=None, local_copies=False, pad_uniform=0, fused=True):
    """search_pipeline over a group of contexts (one per entry of `devices`)"""
    packed = PackedReads(seqs, pad_uniform)
    header_id = None
    if headers is not None:
        first = {}
        header_id = np.empty(len(headers), np.uint64)
        for i, h in enumerate(headers):
            header_id[i] = first.setdefault(h, i)
        if np.all(header_id == np.arange(len(headers), dtype=np.uint64)):
            header_id = None
    g = SearchGroup(devices, params, local_copies)
    try:
        g.load_reads(packed, header_id)
        if fused:
            g.step()
        else:
            g.seed_scan(); g.merge(); g.recruit()
        return g.result()
    finally:
        g.close()
        packed.close()


class PipelineResult:
    """Same field names as tests/orc.PipelineResult so parity tests compare attribute by attribute."""

    def __init__(self, cand, merge, rec, max_read_len):
        self.n_pass1, self.n_pass2 = cand.n, rec.n
        self.n_tokens, self.n_groups, self.n_patterns = merge.n_tokens, merge.n_groups, merge.n_patterns
        self.max_read_len = max_read_len
        self.error = 0
        self.rec_read = np.concatenate([cand.read_idx, rec.read_idx])
        self.rec_lowlexi = np.concatenate([cand.low_lexi, rec.low_lexi])
        self.rec_token = np.concatenate([merge.cand_token[:cand.n] if len(merge.cand_token) == cand.n
                                         else merge.cand_token, rec.token]).astype(np.uint32)
        self.rec_replen = np.concatenate([cand.repeat_len, np.zeros(rec.n, np.uint32)])
        self.rec_nss = np.concatenate([cand.n_ss, np.full(rec.n, 2, np.uint32)])
        rec_ss = np.stack([rec.start, rec.end], axis=1).reshape(-1) if rec.n else np.zeros(0, np.uint32)
        self.ss_pool = np.concatenate([cand.ss_pool, rec_ss]).astype(np.uint32)
        off1 = cand.ss_off
        base = len(cand.ss_pool)
        off2 = base + 2 * np.arange(rec.n, dtype=np.uint64)
        self.rec_ss_off = np.concatenate([off1, off2]).astype(np.uint64)
        self.tokens, self.groups, self.patterns, self.pat_group = merge.tokens, merge.groups, merge.patterns, merge.pat_group
        self.cand, self.merge, self.rec = cand, merge, rec

    def ss(self, k):
        o = int(self.rec_ss_off[k])
        return self.ss_pool[o:o + int(self.rec_nss[k])].tolist()


def search_pipeline(seqs, headers=None, params=None, device=0, do_pass2=True, engine=None, pad_uniform=0):
    """pass 1 -> merge -> pass 2 on one GPU for host reads (list[bytes]); returns PipelineResult.
    pad_uniform: crass_pack_reads' layout switch (0 tight, 1 one stride, 2 automatic)."""
    packed = PackedReads(seqs, pad_uniform)
    header_id = None
    if headers is not None:
        first = {}
        header_id = np.empty(len(headers), np.uint64)
        for i, h in enumerate(headers):
            header_id[i] = first.setdefault(h, i)
        if np.all(header_id == np.arange(len(headers), dtype=np.uint64)):
            header_id = None
    own = engine is None
    eng = engine or SearchEngine(params, device)
    if not own:
        eng.reload_env()                # a reused context re-reads the A/B switches (they are read once per context)
    try:
        eng.load_reads(packed, header_id)
        cand = eng.seed_scan()
        merge = eng.merge()
        if do_pass2:
            rec = eng.recruit()
            merge = eng.merge_view()        # pass 2 may add tokens (addReadHolder)
        else:
            rec = RecruitSet(_abi.Recruits())
        res = PipelineResult(cand, merge, rec, cand.max_read_len)
        res.counters = eng.counters()
        return res
    finally:
        if own:
            eng.close()
        packed.close()


class ConsensusResult:
    """crass_cons_view as numpy / python objects (same field names as the oracle's result in tests/orc.py)"""

    def __init__(self, v):
        def arr(ptr, cnt, dt):
            if cnt == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ptr, shape=(int(cnt),)).astype(dt, copy=True)
        self.error, self.next_free_gid, self.n_tokens = int(v.error), int(v.next_free_gid), int(v.n_tokens)
        off = arr(v.tok_off, v.n_tokens + 1, np.uint64)
        tc = C.string_at(v.tok_chars, int(off[-1])) if v.n_tokens else b""
        self.tokens = [tc[int(off[i]):int(off[i + 1])] for i in range(v.n_tokens)]
        ng = int(v.n_groups)
        self.gids = arr(v.grp_gid, ng, np.int32).tolist()
        doff = arr(v.dr_off, ng + 1, np.uint64)
        dc = C.string_at(v.dr_chars, int(doff[-1])) if ng else b""
        self.true_drs = [dc[int(doff[i]):int(doff[i + 1])] for i in range(ng)]
        goff = arr(v.grp_off, ng + 1, np.uint64)
        gt = arr(v.grp_tokens, int(goff[-1]) if ng else 0, np.uint32)
        self.groups = [gt[int(goff[i]):int(goff[i + 1])].tolist() for i in range(ng)]
        n = int(v.n_rec)
        self.rec_alive = arr(v.rec_alive, n, np.uint8)
        self.rec_rc = arr(v.rec_rc, n, np.uint8)
        self.rec_token = arr(v.rec_token, n, np.uint32)
        self.rec_nss = arr(v.rec_nss, n, np.uint32)
        self.rec_ss_off = arr(v.rec_ss_off, n, np.uint64)
        self.ss_pool = arr(v.ss_pool, int(self.rec_nss.sum()), np.uint32)
        toff = arr(v.tokread_off, v.n_tokens + 1, np.uint64)
        tidx = arr(v.tokread_idx, int(toff[-1]) if v.n_tokens else 0, np.uint64)
        has = arr(v.tok_has_list, v.n_tokens, np.uint8)
        self.reads_of = [tidx[int(toff[i]):int(toff[i + 1])].tolist() if has[i] else None for i in range(v.n_tokens)]
        self.counters = v.counters.asdict()

    def ss(self, k):
        o = int(self.rec_ss_off[k])
        return self.ss_pool[o:o + int(self.rec_nss[k])].tolist()

    def group_read_counts(self):
        return [sum(len(self.reads_of[t - 2] or []) for t in g) for g in self.groups]


def consensus(seqs, res, params=None, device=0):
    """crass_hip_consensus (WorkHorse::findConsensusDRs) over a search result: a PipelineResult of this module or any object
    with its fields (rec_read, rec_lowlexi, rec_token, rec_nss, rec_ss_off, ss_pool, tokens, groups, max_read_len,
    n_pass1, n_pass2).  seqs: list[bytes] or (uint8 array, uint64 offsets) — the input reads."""
    lib = _abi.load()
    p = params or default_params()
    if isinstance(seqs, (list, tuple)) and (not seqs or isinstance(seqs[0], (bytes, bytearray))):
        sbuf, soff = concat(list(seqs))
    else:
        sbuf, soff = seqs
    n = int(res.n_pass1 + res.n_pass2)
    keep = []

    def a(x, dt):
        y = np.ascontiguousarray(np.asarray(x)[:n], dtype=dt)
        keep.append(y)
        return y.ctypes.data
    tbuf, toff = concat(list(res.tokens))
    goff = np.zeros(len(res.groups) + 1, np.uint64)
    goff[1:] = np.cumsum([len(g) for g in res.groups], dtype=np.uint64)
    gt = np.array([t for g in res.groups for t in g], np.uint32)
    ssp = np.ascontiguousarray(res.ss_pool, np.uint32)
    i = _abi.ConsInput(sbuf.ctypes.data, soff.ctypes.data, len(soff) - 1, n, a(res.rec_read, np.uint64), a(res.rec_lowlexi, np.uint8),
                       a(res.rec_token, np.uint32), a(res.rec_nss, np.uint32), a(res.rec_ss_off, np.uint64), ssp.ctypes.data,
                       len(res.tokens), tbuf.ctypes.data, toff.ctypes.data, len(res.groups), gt.ctypes.data, goff.ctypes.data,
                       int(res.max_read_len))
    h = C.c_void_p()
    import time as _time
    _t0 = _time.perf_counter()
    _chk(lib.crass_hip_consensus(C.byref(p), int(device), C.byref(i), C.byref(h)), "crass_hip_consensus")
    consensus.last_call_s = _time.perf_counter() - _t0       # the C call alone (what an adapter pays), without this wrapper's conversions
    try:
        v = _abi.ConsView()
        _chk(lib.crass_hip_consensus_view(h, C.byref(v)), "crass_hip_consensus_view")
        return ConsensusResult(v)
    finally:
        lib.crass_hip_consensus_free(h)


def ksw_batch(cases, device=0):
    """crass_hip_ksw_batch: cases = [(query codes, target codes)] (codes 0..4) -> int32 [n, 2, 3]: (score, tb, qb) of each query
    and of its reverse complement against its target, with the Aligner's scoring"""
    q_off, q_len, t_off, t_len, items, pos = [], [], [], [], [], 0
    for q, _ in cases:
        q_off.append(pos); q_len.append(len(q)); items.append(bytes(q)); pos += len(q)
    qc = np.frombuffer(b"".join(items) + b"\0", np.uint8).copy()
    items, pos = [], 0
    for _, t in cases:
        t_off.append(pos); t_len.append(len(t)); items.append(bytes(t)); pos += len(t)
    tc = np.frombuffer(b"".join(items) + b"\0", np.uint8).copy()
    q_off, q_len, t_off, t_len = (np.array(x, np.uint32) for x in (q_off, q_len, t_off, t_len))
    tgt = np.arange(len(cases), dtype=np.uint32)
    out = np.zeros((len(cases), 2, 3), np.int32)
    _chk(_abi.load().crass_hip_ksw_batch(int(device), qc.ctypes.data, q_off.ctypes.data, q_len.ctypes.data, tgt.ctypes.data, len(cases),
                                         tc.ctypes.data, t_off.ctypes.data, t_len.ctypes.data, len(cases), out.ctypes.data),
         "crass_hip_ksw_batch")
    return out


def smith_waterman_batch(tasks, similarity=0.85, device=0):
    """crass_hip_smith_waterman_batch: tasks = [(read bytes, DR bytes, start, len)] -> (int32 [n, 6] of aStart, aEnd, a_off, a_len,
    b_off, b_len, number of k_cons_sw launches).  a_ret = read[a_off:a_off + a_len], b_ret = DR[b_off:b_off + b_len]"""
    r_off, r_len, d_off, d_len, st, ln, items, pos = [], [], [], [], [], [], [], 0
    for a, b, s, n in tasks:
        r_off.append(pos); r_len.append(len(a)); items.append(bytes(a)); pos += len(a)
        d_off.append(pos); d_len.append(len(b)); items.append(bytes(b)); pos += len(b)
        st.append(s); ln.append(n)
    chars = np.frombuffer(b"".join(items) + b"\0", np.uint8).copy()
    r_off, d_off = np.array(r_off, np.uint64), np.array(d_off, np.uint64)
    r_len, d_len = np.array(r_len, np.uint32), np.array(d_len, np.uint32)
    st, ln = np.array(st, np.int32), np.array(ln, np.int32)
    out = np.zeros((6, len(tasks)), np.int32)
    launches = C.c_uint32(0)
    _chk(_abi.load().crass_hip_smith_waterman_batch(int(device), chars.ctypes.data, pos, r_off.ctypes.data, r_len.ctypes.data, d_off.ctypes.data,
                                                    d_len.ctypes.data, st.ctypes.data, ln.ctypes.data, len(tasks), float(similarity),
                                                    *[out[k].ctypes.data for k in range(6)], C.byref(launches)),
         "crass_hip_smith_waterman_batch")
    return out.T.copy(), launches.value


def build_outputs(groups, out_dir="./", timestamp="", command_line="", cwd="", log_to_screen=True, cov_cutoff=0, write_to=None):
    """crass_build_outputs (WorkHorse::buildGraph ... outputResults): groups = [(gid, true_dr bytes, [(header, comment or None, seq,
    start_stops), ...])] in ascending GID, the reads in buildGraph's order.  Returns (files {name: bytes}, kept gids, stdout text);
    write_to: also write the files into that directory (crass_outputs_write)."""
    lib = _abi.load()
    gid = np.array([g for g, _, _ in groups], np.int32)
    dr_buf, dr_off = concat([d for _, d, _ in groups])
    recs = [r for _, _, rs in groups for r in rs]
    goff = np.zeros(len(groups) + 1, np.uint64)
    if groups:
        goff[1:] = np.cumsum([len(rs) for _, _, rs in groups], dtype=np.uint64)
    hb, ho = concat([r[0] for r in recs])
    cb, co = concat([(r[1] or b"") for r in recs])
    sb, so = concat([r[2] for r in recs])
    nss = np.array([len(r[3]) for r in recs], np.uint32)
    ssoff = np.zeros(len(recs), np.uint64)
    if len(recs) > 1:
        ssoff[1:] = np.cumsum(nss[:-1], dtype=np.uint64)
    pool = np.array([v for r in recs for v in r[3]] or [0], np.uint32)

    def ptr(a):
        return a.ctypes.data if a.size else None
    gi = _abi.GraphInput(len(groups), ptr(gid), ptr(dr_buf), dr_off.ctypes.data, goff.ctypes.data, len(recs), ptr(hb), ho.ctypes.data,
                         ptr(cb) if cb.size else None, co.ctypes.data, ptr(sb), so.ctypes.data, ptr(nss), ptr(ssoff), pool.ctypes.data)
    if cb.size == 0:
        cz = np.zeros(1, np.uint8)                  # (no comment bytes at all: an empty but valid buffer)
        gi.com_chars = cz.ctypes.data
    oo = _abi.OutputOpts(out_dir.encode() if isinstance(out_dir, str) else out_dir, timestamp.encode(), command_line.encode(), cwd.encode(),
                         1 if log_to_screen else 0, int(cov_cutoff), 0, 0, 0)
    h = C.c_void_p()
    _chk(lib.crass_build_outputs(C.byref(gi), C.byref(oo), C.byref(h)), "crass_build_outputs")
    try:
        v = _abi.OutputsView()
        _chk(lib.crass_outputs_get(h, C.byref(v)), "crass_outputs_get")
        files = {v.name[i].decode(): C.string_at(v.data[i], int(v.size[i])) for i in range(v.n_files)}
        kept = [int(v.kept_gid[i]) for i in range(v.n_groups_kept)]
        text = v.stdout_text.decode()
        if write_to is not None:
            _chk(lib.crass_outputs_write(h, str(write_to).encode()), "crass_outputs_write")
        return files, kept, text
    finally:
        lib.crass_outputs_free(h)
