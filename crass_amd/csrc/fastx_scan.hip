// fastx_scan.hip — the record scan of fastx_scan.h on the device: the raw bytes of a FASTA / FASTQ file -> the reads' bytes back
// to back (the text pack.hip packs), the position of every record's header character, the reads' offsets in the text, and one
// verdict word.  Raw bytes -> per-tile summaries -> one scan over the tiles -> emit: TWO passes over the raw bytes.
//
// What a byte means depends on the line it is in (header, sequence, '+', quality), and what a line is depends on everything in
// front of it: FASTA — whether its first byte is '>'; FASTQ — its index modulo 4.  Both are carried as "the last line start in
// front of here" (a tile's function on that is a constant, the tile's own last line start, or the identity, a tile that starts no
// line) and "line starts so far" (a sum), so they scan associatively over tiles:
//   k_fx_summary    one block per tile of kFxTileBytes, a lane one aligned 16-byte vector: line starts, the last one, and the
//                   bytes 33..126 of the tile sorted by what they could turn out to be (FxTile).  24 bytes per tile.
//   k_fx_tile_scan  one block walks the tiles, 1 024 per step: line index, carried line, records / sequence / quality bytes in
//                   front of every tile (FxBase, 48 bytes per tile) and the four totals.  64-bit sums (files beyond 4 GB), which
//                   is why this is not the 32-bit look-back of sinks.hip.
//   k_fx_emit       the tile again, now with its base: sequence bytes go through LDS to the text in aligned 16-byte stores,
//                   every header line start writes rec_pos / seq_off, every offence of fastx_scan.h is min-ed into the verdict.
//                   Several files as one set (crass_hip_load_fastx_files): a launch per file with the file's text base, read
//                   base and arena base, so that all files fill one text, one seq_off and one rec_pos (arena positions).
//   k_fx_cut_probe  (beside the scan, for a group's files load) what a rank knows about a byte range before the cuts are known:
//                   its '\n' bytes, first four line starts and first '>' line start — one pass, one part per block, no atomics.
// Temporary HBM per input byte: 72 / 4096 for the tile arrays, at most 1 for the text, 16 per record for the two arrays.
// No byte beyond the input is read: the first and the last vector are loaded byte by byte where they are not whole.
#include "fastx_vec.h"

namespace crass {

// The lines of a vector in order: f(seg, started, j, kind) for the bytes `seg` of one line — the one that reaches in from the
// left (started false, kind in_kind), then every line that starts in the vector (at bit j).  FASTQ: a line's kind is the one
// before it plus one; FASTA: whether its first byte is '>'.
template <class F> static __device__ __forceinline__ void fx_walk(const FxVec &V, bool fastq, uint32_t in_kind, F f)
{
    uint32_t rem = V.ls;
    const uint32_t first = rem ? (uint32_t)__builtin_ctz(rem) : 16u;
    const uint32_t seg0 = V.valid & ((1u << first) - 1u);
    if (seg0) f(seg0, false, 0u, in_kind);
    uint32_t kind = in_kind;
    while (rem) {
        const uint32_t j = (uint32_t)__builtin_ctz(rem);
        rem &= rem - 1u;
        const uint32_t nxt = rem ? (uint32_t)__builtin_ctz(rem) : 16u;
        const uint32_t seg = V.valid & ((1u << nxt) - 1u) & ~((1u << j) - 1u);
        kind = fastq ? (kind + 1u) & 3u : (((V.gt >> j) & 1u) ? (uint32_t)FX_HEADER : (uint32_t)FX_SEQ);
        f(seg, true, j, kind);
    }
}
// a lane's last line start as a sortable code (FxTile::lls with the offset in the TILE); 0: none
static __device__ __forceinline__ uint32_t fx_last_ls_code(const FxVec &V)
{
    if (!V.ls) return 0u;
    const uint32_t j = 31u - (uint32_t)__builtin_clz(V.ls);
    return ((16u * threadIdx.x + j + 1u) << 1) | ((V.gt >> j) & 1u);
}

__global__ __launch_bounds__(kFxThreads) void k_fx_summary(const FxJob J)
{
    __shared__ uint32_t s_w[kFxThreads / 64];
    __shared__ uint32_t s_acc[6];
    const uint32_t tid = threadIdx.x;
    const uint64_t q0 = (uint64_t)blockIdx.x * kFxTileBytes + 16u * tid;
    const bool fastq = J.format == 0x40;
    if (tid < 6) s_acc[tid] = 0u;                       // (the scans below synchronise before anybody adds)
    FxVec V;
    fx_load(J, q0, V);
    uint32_t tot_ls, tot_code;
    const uint32_t excl = fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.ls), s_w, &tot_ls);
    const uint32_t prev = fx_scan_max<kFxThreads / 64>(fx_last_ls_code(V), s_w, &tot_code);
    // FASTQ: kinds are the lines' indices among the tile's own, modulo 4
    const uint32_t in_kind = fastq ? (excl - 1u) & 3u : ((prev & 1u) ? (uint32_t)FX_HEADER : (uint32_t)FX_SEQ);
    uint32_t cp = 0, lead_g = 0, n_hdr = 0;             // cp: four 8-bit counts (a lane has 16 bytes)
    {                                                   // (fx_walk's order, written out: its captures cost this kernel 12 bytes of scratch)
        uint32_t rem = V.ls, kind = in_kind;
        const uint32_t first = rem ? (uint32_t)__builtin_ctz(rem) : 16u;
        const uint32_t g0 = (uint32_t)__builtin_popcount(V.gr & ((1u << first) - 1u));
        if (prev == 0u) lead_g = g0;
        else if (fastq) cp = g0 << (8u * kind);
        else if (kind == FX_SEQ) cp = g0;
        while (rem) {
            const uint32_t j = (uint32_t)__builtin_ctz(rem);
            rem &= rem - 1u;
            const uint32_t nxt = rem ? (uint32_t)__builtin_ctz(rem) : 16u;
            const uint32_t g = (uint32_t)__builtin_popcount(V.gr & ((1u << nxt) - 1u) & ~((1u << j) - 1u));
            kind = fastq ? (kind + 1u) & 3u : (((V.gt >> j) & 1u) ? (uint32_t)FX_HEADER : (uint32_t)FX_SEQ);
            if (fastq) cp += g << (8u * kind);
            else if (kind == FX_SEQ) cp += g;
            else n_hdr++;
        }
    }
    const uint32_t lo = fx_wave_sum(cp & 0x00FF00FFu), hi = fx_wave_sum((cp >> 8) & 0x00FF00FFu);      // (64 x 16 fits 16 bits)
    lead_g = fx_wave_sum(lead_g); n_hdr = fx_wave_sum(n_hdr);
    if ((tid & 63u) == 0) {
        atomicAdd(&s_acc[0], lo & 0xFFFFu); atomicAdd(&s_acc[1], hi & 0xFFFFu); atomicAdd(&s_acc[2], lo >> 16); atomicAdd(&s_acc[3], hi >> 16);
        atomicAdd(&s_acc[4], lead_g); atomicAdd(&s_acc[5], n_hdr);
    }
    __syncthreads();
    if (tid == 0) {
        FxTile T;
        T.n_ls = tot_ls; T.lls = tot_code; T.lead_g = s_acc[4]; T.n_hdr = s_acc[5];
        T.c01 = s_acc[0] | (s_acc[1] << 16); T.c23 = s_acc[2] | (s_acc[3] << 16);      // (at most 4 096 each)
        J.tiles[blockIdx.x] = T;
    }
}

__global__ __launch_bounds__(kFxScanThreads) void k_fx_tile_scan(const FxJob J)
{
    __shared__ uint32_t s_w[kFxScanThreads / 64];
    __shared__ uint64_t s_pos[kFxScanThreads];
    __shared__ uint32_t s_lls[kFxScanThreads];
    const uint32_t tid = threadIdx.x;
    const bool fastq = J.format == 0x40;
    uint64_t r_ls = 0, r_pos = 0, r_rec = 0, r_seq = 0, r_qual = 0;      // everything in front of this step's tiles (the same in every thread)
    uint32_t r_kind = FX_HEADER;
    for (uint64_t t0 = 0; t0 < J.n_tiles; t0 += kFxScanThreads) {
        const uint64_t t = t0 + tid;
        const bool have = t < J.n_tiles;
        FxTile S{};
        if (have) S = J.tiles[t];
        s_pos[tid] = t * kFxTileBytes - J.lead + (S.lls >> 1) - 1u;      // file position of the tile's last line start
        s_lls[tid] = S.lls;
        uint32_t tot_ls, tot_code, tot_seq, tot_qual, tot_hdr;
        const uint64_t ls_before = r_ls + fx_scan_add<kFxScanThreads / 64>(S.n_ls, s_w, &tot_ls);
        const uint32_t prev = fx_scan_max<kFxScanThreads / 64>(S.lls ? tid + 1u : 0u, s_w, &tot_code);
        const uint64_t carry_ls = prev ? s_pos[prev - 1] : r_pos;
        const uint32_t fa_kind = prev ? ((s_lls[prev - 1] & 1u) ? (uint32_t)FX_HEADER : (uint32_t)FX_SEQ) : r_kind;
        const uint32_t carry_kind = fastq ? (uint32_t)(ls_before - 1u) & 3u : fa_kind;
        const uint32_t c[4] = {S.c01 & 0xFFFFu, S.c01 >> 16, S.c23 & 0xFFFFu, S.c23 >> 16};
        auto pick = [&](uint32_t r) { return r == 0 ? c[0] : r == 1 ? c[1] : r == 2 ? c[2] : c[3]; };
        uint32_t seq, qual = 0, hdr;
        if (fastq) {                                    // the tile's own line j is line ls_before + j of the file
            seq = (carry_kind == FX_SEQ ? S.lead_g : 0u) + pick((uint32_t)(1u - ls_before) & 3u);
            qual = (carry_kind == FX_QUAL ? S.lead_g : 0u) + pick((uint32_t)(3u - ls_before) & 3u);
            const uint32_t j0 = (uint32_t)(0u - ls_before) & 3u;
            hdr = S.n_ls > j0 ? (S.n_ls - j0 + 3u) / 4u : 0u;
        } else {
            seq = (carry_kind == FX_SEQ ? S.lead_g : 0u) + c[0];
            hdr = S.n_hdr;
        }
        FxBase B;
        B.ls_before = ls_before; B.carry_ls = carry_ls; B.carry_kind = carry_kind; B.pad = 0;
        B.seq_before = r_seq + fx_scan_add<kFxScanThreads / 64>(seq, s_w, &tot_seq);
        B.qual_before = r_qual + fx_scan_add<kFxScanThreads / 64>(qual, s_w, &tot_qual);
        B.rec_before = r_rec + fx_scan_add<kFxScanThreads / 64>(hdr, s_w, &tot_hdr);
        if (have) J.base[t] = B;
        if (tot_code) { r_pos = s_pos[tot_code - 1]; r_kind = (s_lls[tot_code - 1] & 1u) ? (uint32_t)FX_HEADER : (uint32_t)FX_SEQ; }
        r_ls += tot_ls; r_seq += tot_seq; r_qual += tot_qual; r_rec += tot_hdr;
        __syncthreads();                                // (s_pos / s_lls are written again)
    }
    if (tid == 0) { J.tot[0] = r_ls; J.tot[1] = r_rec; J.tot[2] = r_seq; J.tot[3] = r_qual; }
}

__global__ __launch_bounds__(kFxThreads) void k_fx_emit(const FxJob J)
{
    __shared__ uint32_t s_w[kFxThreads / 64];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kFxTileBytes + 32];
    const uint32_t tid = threadIdx.x;
    const uint64_t q0 = (uint64_t)blockIdx.x * kFxTileBytes + 16u * tid;
    const uint64_t p0 = q0 - J.lead;                    // file position of the vector's byte 0 (wraps in front of the input: those bytes are not valid)
    const bool fastq = J.format == 0x40;
    const FxBase B = J.base[blockIdx.x];
    FxVec V;
    fx_load(J, q0, V);
    uint32_t tot_ls, tot_code, tot_sq, tot_h;
    const uint32_t excl = fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.ls), s_w, &tot_ls);
    const uint32_t prev = fx_scan_max<kFxThreads / 64>(fx_last_ls_code(V), s_w, &tot_code);
    // the line that reaches into this vector: one of the tile (prev) or the tile's carried one
    const uint64_t in_pos = prev ? (uint64_t)blockIdx.x * kFxTileBytes - J.lead + (prev >> 1) - 1u : B.carry_ls;
    const uint64_t in_idx = B.ls_before + excl - 1u;    // its index (wraps to -1 in front of line 0: no valid byte is there)
    const uint32_t in_kind = fastq ? (uint32_t)in_idx & 3u : (prev ? ((prev & 1u) ? (uint32_t)FX_HEADER : (uint32_t)FX_SEQ) : B.carry_kind);
    // 1. how many sequence bytes, quality bytes and records this lane has
    uint32_t s_cnt = 0, q_cnt = 0, h_cnt = 0, seqmask = 0;
    fx_walk(V, fastq, in_kind, [&](uint32_t seg, bool started, uint32_t, uint32_t kind) {
        const uint32_t g = V.gr & seg;
        if (kind == FX_SEQ) { s_cnt += (uint32_t)__builtin_popcount(g); seqmask |= g; }
        else if (kind == FX_QUAL) q_cnt += (uint32_t)__builtin_popcount(g);
        if (started && kind == FX_HEADER) h_cnt++;
    });
    const uint32_t sq = fx_scan_add<kFxThreads / 64>(s_cnt | (q_cnt << 16), s_w, &tot_sq);      // (a tile has at most 4 096 of either)
    const uint32_t h_excl = fx_scan_add<kFxThreads / 64>(h_cnt, s_w, &tot_h);
    // 2. records and offences
    uint32_t s_run = sq & 0xFFFFu, q_run = sq >> 16, h_run = h_excl;
    uint64_t gidx = in_idx;
    uint64_t off = kFxNoOffence;
    const uint64_t last_q = (uint64_t)J.lead + J.n - 1u;       // the input's last byte in aligned space
    const uint32_t last_bit = (last_q >= q0 && last_q < q0 + 16) ? 1u << (uint32_t)(last_q - q0) : 0u;
    uint64_t ls_pos = in_pos;
    fx_walk(V, fastq, in_kind, [&](uint32_t seg, bool started, uint32_t j, uint32_t kind) {
        auto offend = [&](uint32_t reason) { const uint64_t o = fx_offence(ls_pos, reason); if (o < off) off = o; };
        if (started) {
            ls_pos = p0 + j; gidx++;
            if (kind == FX_HEADER) {
                const uint64_t r = B.rec_before + h_run++;
                if (r < J.n_reads) { J.rec_pos[J.read_base + r] = J.arena_base + ls_pos; J.seq_off[J.read_base + r] = J.text_base + B.seq_before + s_run; }
                if (fastq) {
                    if ((J.n_lines & 3u) && gidx == (J.n_lines & ~3ull)) offend(FX_LINE_COUNT);
                    if (!((V.at >> j) & 1u)) offend(FX_FQ_HEADER);
                } else if (ls_pos == J.n - 1u) offend(FX_LONE_HEADER);
            } else if (kind == FX_PLUS && !((V.pl >> j) & 1u)) offend(FX_FQ_PLUS);
        }
        if (kind == FX_SEQ) {
            if ((V.gt | V.at | V.pl) & seg) offend(FX_SEQ_CHAR);
            s_run += (uint32_t)__builtin_popcount(V.gr & seg);
        } else if (kind == FX_QUAL) {
            if (V.del & seg) offend(FX_QUAL_DEL);
            q_run += (uint32_t)__builtin_popcount(V.gr & seg);
            if ((V.nl | last_bit) & seg) {              // the line ends here: sequence and quality bytes so far must be as many
                const uint64_t S = B.seq_before + s_run, Q = B.qual_before + q_run;
                if (S > Q) offend(FX_QUAL_SHORT);
                if (S < Q) offend(FX_QUAL_LONG);
            }
        }
    });
    if (off != kFxNoOffence) atomicMin(J.verdict, (unsigned long long)off);
    // 3. the tile's sequence bytes: into LDS where they will lie relative to the text's 16-byte vectors, then out
    const uint64_t t0 = J.text_base + B.seq_before;    // where the tile's first sequence byte goes in the text
    const uint32_t shift = (uint32_t)(t0 & 15u);
    {
        uint32_t o = shift + (sq & 0xFFFFu);
#pragma unroll
        for (int j = 0; j < 16; j++) if ((seqmask >> j) & 1u) { if (o < kFxTileBytes + 32u) s_out[o] = (uint8_t)(V.w[j >> 2] >> (8 * (j & 3))); o++; }
    }
    __syncthreads();
    const uint32_t n_out = shift + (tot_sq & 0xFFFFu);  // LDS bytes [shift, n_out) are the tile's
    const uint64_t g0 = t0 - shift;           // text offset of LDS byte 0 (a multiple of 16)
    for (uint32_t v = tid; 16u * v < n_out; v += kFxThreads) {
        const uint32_t a = 16u * v, b = a + 16u;
        if (a >= shift && b <= n_out && g0 + b <= J.text_cap) {
            *reinterpret_cast<uint4 *>(J.text + g0 + a) = *reinterpret_cast<const uint4 *>(s_out + a);
        } else {                                        // (the vector the tile shares with the one before or behind it)
            for (uint32_t i = a > shift ? a : shift; i < b && i < n_out; i++) if (g0 + i < J.text_cap) J.text[g0 + i] = s_out[i];
        }
    }
}

// The probe of fastx_scan.h over a byte range: a stream, one aligned 16-byte load per 16 bytes (fx_load: the range's first and
// last vector byte by byte where they are not whole, so no byte outside the range is even loaded).  Block b walks the tiles
// [b tiles_per_block, (b + 1) tiles_per_block) in order and writes ONE FxProbe of its own: the '\n' bytes of its tiles, their
// first four line starts and their first '>' line start, positions from the range's first byte.  The blocks' parts are folded
// in block order (fx_probe_fold), so every minimum is one by position: nothing depends on which block ran first, and there is
// no atomic.
__global__ __launch_bounds__(kFxThreads) void k_fx_cut_probe(const FxProbeJob P)
{
    __shared__ uint32_t s_w[kFxThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    FxJob J{};
    J.bytes = P.bytes; J.n = P.n; J.lead = P.lead;      // (what fx_load reads of a job)
    const uint64_t t_begin = (uint64_t)blockIdx.x * P.tiles_per_block;
    const uint64_t t_end = t_begin + P.tiles_per_block < P.n_tiles ? t_begin + P.tiles_per_block : P.n_tiles;
    FxProbe *out = P.part + blockIdx.x;
    if (tid == 0) { out->ls[0] = out->ls[1] = out->ls[2] = out->ls[3] = kFxNone; }
    __syncthreads();
    uint32_t nl_cnt = 0, found = 0;                     // found: the block's line starts so far (the same in every thread)
    uint64_t gt = kFxNone;                              // (the same in every thread)
    for (uint64_t t = t_begin; t < t_end; t++) {
        const uint64_t q0 = t * kFxTileBytes + 16u * tid;
        FxVec V;
        fx_load(J, q0, V);
        // fx_load takes the input's position 0 for a line start; here the caller says whether it is one
        if (!P.left_is_ls && P.lead >= q0 && P.lead < q0 + 16) V.ls &= ~(1u << (uint32_t)(P.lead - q0));
        nl_cnt += (uint32_t)__builtin_popcount(V.nl);
        if (found < 4u) {
            uint32_t tot;
            uint32_t k = found + fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.ls), s_w, &tot);
            for (uint32_t rem = V.ls; rem && k < 4u; rem &= rem - 1u) out->ls[k++] = q0 - P.lead + (uint32_t)__builtin_ctz(rem);
            found += tot;
        }
        if (gt == kFxNone) {
            const uint32_t m = V.ls & V.gt;
            uint32_t code = m ? 16u * tid + (uint32_t)__builtin_ctz(m) : 0xFFFFFFFFu;      // offset in the tile
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)code, s); code = y < code ? y : code; }
            if (lane == 0) s_w[wv] = code;
            __syncthreads();
            uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < kFxThreads / 64; k++) mn = s_w[k] < mn ? s_w[k] : mn;
            __syncthreads();
            if (mn != 0xFFFFFFFFu) gt = t * kFxTileBytes - P.lead + mn;
        }
    }
    uint32_t tot_nl;
    (void)fx_scan_add<kFxThreads / 64>(nl_cnt, s_w, &tot_nl);      // (the launch keeps a block's tiles below 4 GB)
    if (tid == 0) { out->n_nl = tot_nl; out->n_ls = found < 4u ? found : 4u; out->gt = gt; }
}

// the blocks' parts in block order -> the range's probe
void fx_probe_fold(const FxProbe *part, uint32_t n_blocks, FxProbe *out)
{
    FxProbe R{};
    R.gt = kFxNone;
    for (int k = 0; k < 4; k++) R.ls[k] = kFxNone;
    for (uint32_t b = 0; b < n_blocks; b++) {
        R.n_nl += part[b].n_nl;
        for (uint64_t k = 0; k < part[b].n_ls && R.n_ls < 4; k++) R.ls[R.n_ls++] = part[b].ls[k];
        if (R.gt == kFxNone) R.gt = part[b].gt;
    }
    *out = R;
}

// the grid of a probe over n bytes at this address: at most kFxProbeMaxBlocks blocks of as many tiles each
void fx_probe_plan(const uint8_t *bytes, uint64_t n, uint32_t left_is_ls, FxProbeJob *P)
{
    *P = FxProbeJob{};
    P->bytes = bytes; P->n = n; P->lead = (uint32_t)((uintptr_t)bytes & 15u); P->left_is_ls = left_is_ls ? 1u : 0u;
    P->n_tiles = fastx_n_tiles(bytes, n);
    P->tiles_per_block = (P->n_tiles + kFxProbeMaxBlocks - 1) / kFxProbeMaxBlocks;
    if (!P->tiles_per_block) P->tiles_per_block = 1;
    P->n_blocks = (uint32_t)((P->n_tiles + P->tiles_per_block - 1) / P->tiles_per_block);
}

hipError_t launch_fx_cut_probe(const FxProbeJob &P, hipStream_t st)
{
    if (!P.n || !P.n_blocks || !P.part || P.tiles_per_block > (0xFFFFFFFFull / kFxTileBytes)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_fx_cut_probe, dim3(P.n_blocks), dim3(kFxThreads), 0, st, P);
    return hipGetLastError();
}

uint32_t fastx_tile_bytes() { return kFxTileBytes; }

uint64_t fastx_n_tiles(const uint8_t *bytes, uint64_t n)
{
    return (((uint64_t)((uintptr_t)bytes & 15u)) + n + kFxTileBytes - 1) / kFxTileBytes;
}

hipError_t launch_fx_summary(const FxJob &J, hipStream_t st)
{
    if (!J.n_tiles || J.n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_fx_summary, dim3((unsigned)J.n_tiles), dim3(kFxThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_fx_tile_scan(const FxJob &J, hipStream_t st)
{
    CRASS_LAUNCH(k_fx_tile_scan, dim3(1), dim3(kFxScanThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_fx_emit(const FxJob &J, hipStream_t st)
{
    if (!J.n_tiles || J.n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_fx_emit, dim3((unsigned)J.n_tiles), dim3(kFxThreads), 0, st, J);
    return hipGetLastError();
}

} // namespace crass
