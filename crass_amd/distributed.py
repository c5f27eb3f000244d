"""Multi-GPU exchange step: one rank per GPU (torch.distributed, backend "nccl" = RCCL over
xGMI on ROCm; "gloo" in the CPU tests).

The path shards by contiguous read ranges; the ONLY data-path exchange is the all-gather of
the pass-1 candidates' representative DR strings between the seed pass and the merge
(SURVEY §8e).  Rank order == global read order, so every rank replays the same
addReadHolder token order and builds the identical pattern list locally — no broadcast of
tables.  Payload: <= a few 10^4 candidates x (stride + 2) bytes, i.e. latency-bound.

A job whose shards share header NAMES (paired files, one per rank) asks for a second exchange,
FoundNameExchange, between the merge and pass 2: the names of every rank's pass-1 reads, so
that a read whose name was found elsewhere is not recruited (readsFound, libcrispr.cpp:411).
A caller that does not ask for it pays no collective for it.
"""
import numpy as np


def allgather_candidates(chars, lens, dist, device=None):
    """chars: uint8 [n_local, stride], lens: uint16 [n_local]  ->  (uint8 [n_global, stride],
    uint16 [n_global]) concatenated in rank order.  Two collectives: counts, then fixed-size
    padded slots (all_gather needs equal shapes)."""
    import torch
    world = dist.get_world_size()
    dev = device if device is not None else torch.device("cpu")
    stride = int(chars.shape[1]) if chars.ndim == 2 and chars.shape[0] else None
    meta = torch.tensor([int(chars.shape[0]), stride or 0], dtype=torch.int64, device=dev)
    metas = [torch.zeros_like(meta) for _ in range(world)]
    dist.all_gather(metas, meta)
    counts = [int(m[0].item()) for m in metas]
    strides = {int(m[1].item()) for m in metas if int(m[0].item()) > 0}
    if not strides:
        return np.zeros((0, 16), np.uint8), np.zeros(0, np.uint16)
    assert len(strides) == 1, "ranks disagree on the DR slot stride"
    stride = strides.pop()
    cap = max(counts)
    slot = stride + 2                                   # DR bytes + uint16 length
    buf = np.zeros((cap, slot), dtype=np.uint8)
    n = int(chars.shape[0])
    if n:
        buf[:n, :stride] = chars
        buf[:n, stride:] = lens.astype("<u2").view(np.uint8).reshape(n, 2)
    send = torch.from_numpy(buf).to(dev)
    recv = [torch.empty_like(send) for _ in range(world)]
    dist.all_gather(recv, send)
    parts_c, parts_l = [], []
    for r in range(world):
        a = recv[r][:counts[r]].cpu().numpy()
        parts_c.append(a[:, :stride])
        parts_l.append(np.ascontiguousarray(a[:, stride:]).view("<u2").reshape(-1).astype(np.uint16))
    return np.ascontiguousarray(np.concatenate(parts_c, axis=0)), np.concatenate(parts_l)


def allgather_distinct(chars, lens, dist, device=None):
    """Compact exchange: every rank contributes only its DISTINCT candidate strings (first-occurrence
    order).  Returns (global chars, global lens, offset of this rank's list in the concatenation)."""
    g_chars, g_lens = allgather_candidates(chars, lens, dist, device)
    counts = gather_counts([int(chars.shape[0])], dist, device)
    my_off = sum(c[0] for c in counts[:dist.get_rank()])
    return g_chars, g_lens, my_off


def gather_counts(values, dist, device=None):
    """small helper: all-gather a list of python ints -> [world][len(values)]"""
    import torch
    dev = device if device is not None else torch.device("cpu")
    t = torch.tensor(list(values), dtype=torch.int64, device=dev)
    out = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [o.cpu().tolist() for o in out]


class _DevView:
    """a device buffer of the engine as a __cuda_array_interface__ object (torch.as_tensor makes a view of it)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def allgather_distinct_device(eng, dist, device):
    """The exchange with everything left on the device (backend "nccl" = RCCL over xGMI): every rank contributes
    its distinct candidate strings straight from the engine's device buffers; the rank-ordered concatenation
    comes back as two device tensors (uint8 [n_global, stride] and uint8 [n_global, 2] = the uint16 lengths).
    Returns (g_chars, g_lens, my_offset) or None when this rank's list is not on the device (the caller then
    uses allgather_distinct with host arrays — every rank must take the same branch, see agree_all)."""
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    dd = eng.distinct_device()
    ok = torch.tensor([1 if dd is not None else 0], dtype=torch.int32, device=device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 0:
        return None
    p_chars, p_len, n, stride = dd
    meta = torch.tensor([n, stride], dtype=torch.int64, device=device)
    metas = torch.empty((world, 2), dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(metas, meta)
    metas = metas.cpu()
    counts = [int(metas[r, 0]) for r in range(world)]
    strides = {int(metas[r, 1]) for r in range(world)}
    assert len(strides) == 1, "ranks disagree on the DR slot stride"
    cap = max(max(counts), 1)
    slot = stride + 2                                   # DR bytes + the uint16 length as two bytes: ONE collective
    send = torch.zeros((cap, slot), dtype=torch.uint8, device=device)
    if n:
        send[:n, :stride] = torch.as_tensor(_DevView(p_chars, (n, stride), "|u1"), device=device)
        send[:n, stride:] = torch.as_tensor(_DevView(p_len, (n, 2), "|u1"), device=device)
    recv = torch.empty((world, cap, slot), dtype=torch.uint8, device=device)
    dist.all_gather_into_tensor(recv, send)
    cat = torch.cat([recv[r, :counts[r]] for r in range(world)])
    g_chars = cat[:, :stride].contiguous()
    g_lens = cat[:, stride:].contiguous()               # [n_global, 2] bytes == uint16 little endian
    torch.cuda.current_stream(device).synchronize()         # the engine reads them on its own stream
    return g_chars, g_lens, sum(counts[:rank])


class GatheredExchange:
    """The exchange as ONE collective per step (RCCL all-gather of fixed-size device buffers).  The engine's seed
    scan leaves the rank's distinct list in its send buffer; step() all-gathers it and merges on the device.
    The row capacity adapts: when some rank's list does not fit (every rank learns that from the gathered
    headers) the buffers are enlarged and the caller repeats the seed scan."""

    def __init__(self, eng, dist, device, cap_rows=0, deferred=True):
        self.eng, self.dist, self.device = eng, dist, device
        self.world, self.rank = dist.get_world_size(), dist.get_rank()
        self._ev = None
        # deferred: eng.seed_scan() returns with pass 1 still queued, the collective is issued with the ENGINE's stream as torch's
        # current stream (the process group orders itself against the current stream on both sides), merge_gathered queues its
        # kernels behind it — no host wait and no idle device between pass 1 and the exchange (crass_hip_exchange_set_deferred)
        self.deferred = bool(deferred)
        self._ext = None
        if not cap_rows:
            # the same capacity on every rank, from the LARGEST shard (crass_hip_exchange_rows_for: the engine's own first-call
            # bound for a shard's distinct DR strings), so that the first step does not overflow and repeat pass 1
            import torch
            n = torch.tensor([int(eng.counters()["n_reads"])], dtype=torch.int64, device=device)
            dist.all_reduce(n, op=dist.ReduceOp.MAX)
            cap_rows = int(eng.lib.crass_hip_exchange_rows_for(int(n.item())))
        self._setup(cap_rows)
        # bring the communicator up now (RCCL initialises lazily on the first collective): not inside a timed step
        import torch
        self.dist.all_gather_into_tensor(self.recv, self.send)
        torch.cuda.current_stream(self.device).synchronize()

    def _setup(self, cap_rows):
        import torch
        self.cap_rows = int(cap_rows)
        ptr, nbytes = self.eng.exchange_setup(self.world, self.rank, self.cap_rows)
        self.send = torch.as_tensor(_DevView(ptr, (nbytes,), "|u1"), device=self.device)
        self.recv = torch.empty((self.world * nbytes,), dtype=torch.uint8, device=self.device)
        if self.deferred:
            if self._ext is None:
                self._ext = torch.cuda.ExternalStream(int(self.eng.stream_handle()), device=self.device)
            torch.cuda.current_stream(self.device).synchronize()      # (recv's allocation belongs to the stream that was current)
            self.eng.exchange_set_deferred(True)

    def step(self):
        """after eng.seed_scan(): True when merged, False when the capacity was raised (repeat the seed scan)"""
        import torch
        if self.deferred:
            with torch.cuda.stream(self._ext):
                self.dist.all_gather_into_tensor(self.recv, self.send)
        else:
            self.dist.all_gather_into_tensor(self.recv, self.send)
            # the engine reads recv on its own stream: ordered behind the collective by an event, no host wait
            if self._ev is None:
                self._ev = torch.cuda.Event()
            self._ev.record(torch.cuda.current_stream(self.device))
            self.eng.stream_wait_event(self._ev.cuda_event)
        need = self.eng.merge_gathered(self.recv.data_ptr(), fetch=False)
        if need is None:
            return True
        cap = self.cap_rows
        while cap < need * 2:
            cap *= 2
        self._setup(cap)
        return False


def allgather_bytes(chars, off, dist, device=None):
    """chars: uint8 [off[-1]], off: uint64 [n + 1] (n byte strings back to back)  ->  a list, per rank, of (chars, off).  The
    pattern of allgather_candidates: counts first, then padded buffers of equal shape (lengths, then bytes)."""
    import torch
    world = dist.get_world_size()
    dev = device if device is not None else torch.device("cpu")
    chars = np.ascontiguousarray(chars, dtype=np.uint8).reshape(-1)
    lens = np.diff(np.ascontiguousarray(off, dtype=np.uint64).astype(np.int64))
    meta = torch.tensor([len(lens), len(chars)], dtype=torch.int64, device=dev)
    metas = [torch.zeros_like(meta) for _ in range(world)]
    dist.all_gather(metas, meta)
    counts = [(int(m[0].item()), int(m[1].item())) for m in metas]
    cap_n, cap_b = max(c[0] for c in counts), max(c[1] for c in counts)
    if cap_n == 0:
        return [(np.zeros(0, np.uint8), np.zeros(1, np.uint64)) for _ in range(world)]
    buf = np.zeros(8 * cap_n + cap_b, dtype=np.uint8)      # [cap_n] int64 lengths, then the bytes
    buf[:8 * len(lens)] = lens.astype("<i8").view(np.uint8)
    buf[8 * cap_n:8 * cap_n + len(chars)] = chars
    send = torch.from_numpy(buf).to(dev)
    recv = [torch.empty_like(send) for _ in range(world)]
    dist.all_gather(recv, send)
    out = []
    for r in range(world):
        a = recv[r].cpu().numpy()
        n, nb = counts[r]
        o = np.zeros(n + 1, np.uint64)
        o[1:] = np.cumsum(np.ascontiguousarray(a[:8 * n]).view("<i8"))
        assert int(o[-1]) == nb, "a rank's name lengths do not add up to its byte count"
        out.append((a[8 * cap_n:8 * cap_n + nb].copy(), o))
    return out


class FoundNameExchange:
    """The found-header exchange of the one-process-per-GPU launcher ("with duplicate headers across shards the
    found-header set must also be exchanged").  Every rank holds its shard's file bytes on the device and has installed its local
    header ids; the name table of those bytes is built here, or by the caller (eng.names_build).  Between the merge and
    eng.recruit every rank calls extra_found with the LOCAL record numbers of its pass-1 reads (ranks that found nothing
    too: the call is collective, two all-gathers):

        xf = FoundNameExchange(eng, dist)
        cand = eng.seed_scan(); ...exchange, merge...
        rec = eng.recruit(extra_found=xf.extra_found(cand.read_idx - base, src, layout))

    Works with gloo (host tensors) and nccl (pass the rank's device)."""

    def __init__(self, eng, dist, device=None, read_index_base=0):
        self.eng, self.dist, self.device = eng, dist, device
        self.read_index_base = int(read_index_base)

    def extra_found(self, found_local_idx, src, layout, job_level=False, build=True):
        """found_local_idx: LOCAL record numbers of this rank's pass-1 reads; src, layout: what fetch_header_lines takes.
        Returns the sorted unique LOCAL record numbers (uint64) of the first record of every name that some OTHER rank found in
        pass 1 — the array eng.recruit(extra_found=...) takes, which marks their header ids found.  job_level: the same with
        read_index_base added (the job's read numbering, e.g. for SearchGroup.recruit).  build=False: the caller has built the
        name table on these bytes (eng.names_build(src, layout)) and nothing has dropped it since; else it is built here, which
        costs well under a millisecond per million reads."""
        eng = self.eng
        if build:
            eng.names_build(src, layout)
        idx = np.unique(np.asarray(found_local_idx, dtype=np.uint64).reshape(-1))
        chars, off, name_len = eng.fetch_header_lines(src, layout, idx)
        # the lines cut at name_len, back to back
        n_off = np.zeros(len(idx) + 1, np.uint64)
        n_off[1:] = np.cumsum(name_len.astype(np.uint64))
        n_chars = np.zeros(int(n_off[-1]), np.uint8)
        for k in range(len(idx)):
            a = int(off[k])
            n_chars[int(n_off[k]):int(n_off[k + 1])] = chars[a:a + int(name_len[k])]
        parts = allgather_bytes(n_chars, n_off, self.dist, self.device)
        rank = self.dist.get_rank()
        others = set()
        for r, (c, o) in enumerate(parts):
            if r == rank:
                continue
            b = c.tobytes()
            others.update(b[int(o[k]):int(o[k + 1])] for k in range(len(o) - 1))
        if not others:
            return np.zeros(0, np.uint64)
        from . import _abi
        first = eng.names_find(sorted(others))
        first = np.unique(first[first != np.uint64(_abi.NAME_NOT_FOUND)])
        return first + np.uint64(self.read_index_base) if job_level else first
