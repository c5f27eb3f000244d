// fastx_wrapped.hip — the wrapped FASTQ rule of fastx_scan.h on the device: records whose sequence and quality run over several
// lines, void lines between records and at the end.  A line's kind is no function of its index here: where a record ends depends
// on a count carried from its sequence, and a quality line may start with '@'.  So the scan is over LINES, not tiles:
//   k_fw_summary    one block per tile of kFxTileBytes (fastx_vec.h): the tile's line starts, those whose byte is '+', and its
//                   bytes 33..126, 127 and '>' '@' '+' (FwTile)
//   k_fw_tile_scan  one block walks the tiles, 1 024 per step: the same counts in front of every tile, 64-bit (FwBase), the totals
//   k_fw_lines      the tile again with its base: one entry per line start — position, first byte, the three counts in front of
//                   the line — and the indices of the '+' lines, compacted in order
//   k_fw_next       a lane per line.  A line whose first byte is '@' is a header CANDIDATE: its '+' line by bisection in the
//                   compacted list, its sequence bytes as a difference of counts, the end of its quality and the next line that
//                   is not void by bisection in the counts; out come its successor, its sequence length and its offence word.
//                   A candidate that offends points at END, as every other line does.
//   k_fw_jump       reachability from line 0 by pointer doubling: per round every marked line marks its successor, then every
//                   line's successor becomes the successor's successor (two arrays in turns).  After round k the first 2^k
//                   records are marked; the launcher runs ceil(log2(lines)) + 1 rounds whatever the data.  Marks are set in
//                   place: a lane may see a mark of its own round, which only marks a reachable line earlier — after the last
//                   round the marked lines are exactly the reachable ones under every schedule.
//   k_fw_rank_*     three launches (tiles, top, apply, as k_nm_scan_* of fastx_lines.hip): a marked line's record index and the
//                   sequence bytes in front of it, 64-bit sums; the records' header lines in order; the verdict, the smallest
//                   offence word of a marked line (only the last reachable record can have one)
//   k_fw_place      a lane per line: a marked line writes rec_pos / seq_off; every line looks up the last header at or in front
//                   of it (bisection in the records' header lines) and, if it lies between that header and its '+' line, where
//                   its bytes go
//   k_fw_emit       the tile once more: a byte 33..126 of such a line is stored at text_base + seq_off + (the bytes 33..126 in
//                   front of it - those in front of its record's first sequence line), a lane its own 16 bytes
//   k_fw_cut_*      the cut of a group's files load: the same rule as a chain to where it leaves a piece (below)
// No block waits for another; every array index is checked against n_lines, every store into the text against its range.
// Scratch: 72 bytes per tile and about 90 per line (fw_scratch_words), the caller's.
#include "fastx_vec.h"

namespace crass {

static __device__ __forceinline__ FxJob fw_as_fx(const FwJob &J)
{
    FxJob X{};
    X.bytes = J.bytes; X.n = J.n; X.lead = J.lead;      // (what fx_load reads of a job)
    return X;
}

__global__ __launch_bounds__(kFxThreads) void k_fw_summary(const FwJob J)
{
    __shared__ uint32_t s_w[kFxThreads / 64];
    const uint64_t q0 = (uint64_t)blockIdx.x * kFxTileBytes + 16u * threadIdx.x;
    FxVec V;
    fx_load(fw_as_fx(J), q0, V);
    uint32_t a, b, f;                                   // (a tile has at most 4 096 of each: two counts share a word)
    (void)fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.ls) | ((uint32_t)__builtin_popcount(V.ls & V.pl) << 16), s_w, &a);
    (void)fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.gr) | ((uint32_t)__builtin_popcount(V.del) << 16), s_w, &b);
    (void)fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.gt | V.at | V.pl), s_w, &f);
    if (threadIdx.x == 0) {
        FwTile T;
        T.n_ls = a & 0xFFFFu; T.n_pl = a >> 16; T.g = b & 0xFFFFu; T.d = b >> 16; T.f = f;
        J.tiles[blockIdx.x] = T;
    }
}

__global__ __launch_bounds__(kFxScanThreads) void k_fw_tile_scan(const FwJob J)
{
    __shared__ uint32_t s_w[kFxScanThreads / 64];
    FwBase r{};                                         // everything in front of this step's tiles (the same in every thread)
    for (uint64_t t0 = 0; t0 < J.n_tiles; t0 += kFxScanThreads) {
        const uint64_t t = t0 + threadIdx.x;
        FwTile S{};
        if (t < J.n_tiles) S = J.tiles[t];
        uint32_t t_ls, t_pl, t_g, t_d, t_f;             // (1 024 tiles of at most 4 096 each fit 32 bits)
        FwBase B;
        B.ls = r.ls + fx_scan_add<kFxScanThreads / 64>(S.n_ls, s_w, &t_ls);
        B.pl = r.pl + fx_scan_add<kFxScanThreads / 64>(S.n_pl, s_w, &t_pl);
        B.g = r.g + fx_scan_add<kFxScanThreads / 64>(S.g, s_w, &t_g);
        B.d = r.d + fx_scan_add<kFxScanThreads / 64>(S.d, s_w, &t_d);
        B.f = r.f + fx_scan_add<kFxScanThreads / 64>(S.f, s_w, &t_f);
        if (t < J.n_tiles) J.base[t] = B;
        r.ls += t_ls; r.pl += t_pl; r.g += t_g; r.d += t_d; r.f += t_f;
    }
    if (threadIdx.x == 0) { J.tot[0] = r.ls; J.tot[1] = r.pl; J.tot[2] = r.g; J.tot[3] = r.d; J.tot[4] = r.f; }
}

__global__ __launch_bounds__(kFxThreads) void k_fw_lines(const FwJob J)
{
    __shared__ uint32_t s_w[kFxThreads / 64];
    const uint64_t q0 = (uint64_t)blockIdx.x * kFxTileBytes + 16u * threadIdx.x;
    const uint64_t p0 = q0 - J.lead;                    // file position of the vector's byte 0 (wraps in front of the input: no line starts there)
    const FwBase B = J.base[blockIdx.x];
    FxVec V;
    fx_load(fw_as_fx(J), q0, V);
    const uint32_t forb = V.gt | V.at | V.pl;
    uint32_t tot;
    const uint32_t a = fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.ls) | ((uint32_t)__builtin_popcount(V.ls & V.pl) << 16), s_w, &tot);
    const uint32_t b = fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.gr) | ((uint32_t)__builtin_popcount(V.del) << 16), s_w, &tot);
    const uint32_t f = fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(forb), s_w, &tot);
    uint64_t li = B.ls + (a & 0xFFFFu), pi = B.pl + (a >> 16);
    const uint64_t g0 = B.g + (b & 0xFFFFu), d0 = B.d + (b >> 16), f0 = B.f + f;
    for (uint32_t rem = V.ls; rem; rem &= rem - 1u, li++) {
        const uint32_t j = (uint32_t)__builtin_ctz(rem), below = (1u << j) - 1u;
        if (li >= J.n_lines) break;
        J.pos[li] = p0 + j;
        J.first[li] = (uint8_t)(V.w[j >> 2] >> (8 * (j & 3)));
        J.G[li] = g0 + (uint32_t)__builtin_popcount(V.gr & below);
        J.D[li] = d0 + (uint32_t)__builtin_popcount(V.del & below);
        J.F[li] = f0 + (uint32_t)__builtin_popcount(forb & below);
        if ((V.pl >> j) & 1u) { if (pi < J.n_lines) J.plus[pi] = (uint32_t)li; pi++; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { J.pos[J.n_lines] = J.n; J.G[J.n_lines] = J.tot[2]; J.D[J.n_lines] = J.tot[3]; J.F[J.n_lines] = J.tot[4]; }
}

// the smallest k in [a, b) with X[k + 1] > X[a]; there is one
static __device__ __forceinline__ uint32_t fw_first_rise(const uint64_t *X, uint32_t a, uint32_t b)
{
    const uint64_t x0 = X[a];
    uint32_t lo = a, hi = b - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (X[mid + 1u] > x0) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

// one header candidate (line i, whose first byte is '@') under the rule of fastx_scan.h, offences in the rule's order.  open:
// what came out depended on where the bytes END — no '+' line, a '+' line that is the last and may be cut, a quality count not
// reached or reached in the last line, no line behind the quality that is not void.  At a file's end that is the rule's "end of
// the input"; at the end of a staged piece it is not known yet (k_fw_cut_next)
struct FwCand { uint32_t nxt, plus_of; uint64_t L, off; bool open; };
static __device__ __forceinline__ FwCand fw_candidate(const FwJob &J, const uint32_t i)
{
    const uint32_t END = J.n_lines;
    FwCand C{END, END, 0, kFxNoOffence, false};
    const uint32_t n_plus = (uint32_t)(J.tot[1] < END ? J.tot[1] : END);
    uint32_t lo = 0, hi = n_plus;                       // the first '+' line behind line i
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (J.plus[mid] > i) hi = mid; else lo = mid + 1u;
    }
    if (lo == n_plus) { C.off = fx_offence(J.pos[i], FX_LINE_COUNT); C.open = true; return C; }
    const uint32_t j = C.plus_of = J.plus[lo];
    const uint64_t L = C.L = J.G[j] - J.G[i + 1u];
    const bool plus_ended = j + 1u < END || J.ends_nl;
    bool short_q = !plus_ended;
    uint32_t q = END;                                   // the first line behind the quality
    if (plus_ended) {
        if (J.G[END] - J.G[j + 1u] < L) short_q = true;
        else {
            uint32_t a = j + 1u, b = END;
            while (a < b) {
                const uint32_t mid = a + ((b - a) >> 1);
                if (J.G[mid] - J.G[j + 1u] >= L) b = mid; else a = mid + 1u;
            }
            q = a;
        }
    }
    C.open = short_q || q == END;
    if (J.F[j] > J.F[i + 1u]) { C.off = fx_offence(J.pos[fw_first_rise(J.F, i + 1u, j)], FX_SEQ_CHAR); C.open = false; }
    else if (L == 0 && j + 1u < END && J.first[j + 1u] == 0x40) { C.off = fx_offence(J.pos[j + 1u], FX_FQ_EMPTY_SEQ); C.open = false; }
    else if (J.D[q] > J.D[j + 1u]) C.off = fx_offence(J.pos[fw_first_rise(J.D, j + 1u, q)], FX_QUAL_DEL);
    else if (!short_q && J.G[q] - J.G[j + 1u] > L) C.off = fx_offence(J.pos[q - 1u], FX_QUAL_LONG);
    else if (short_q) C.off = fx_offence(J.pos[i], FX_QUAL_SHORT);
    else {
        const uint64_t gd = J.G[q] + J.D[q];
        if (J.G[END] + J.D[END] > gd) {                 // the first line at or behind q that is not void
            uint32_t a = q, b = END - 1u;
            while (a < b) {
                const uint32_t mid = a + ((b - a) >> 1);
                if (J.G[mid + 1u] + J.D[mid + 1u] > gd) b = mid; else a = mid + 1u;
            }
            if (J.first[a] == 0x40) C.nxt = a; else C.off = fx_offence(J.pos[a], FX_FQ_HEADER);
        } else C.open = true;
    }
    return C;
}

// A candidate that offends points at END, as every other line does.
__global__ __launch_bounds__(kFxThreads) void k_fw_next(const FwJob J)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    const uint32_t END = J.n_lines;
    if (i64 > END) return;
    const uint32_t i = (uint32_t)i64;
    if (i == END) { J.nxt[0][END] = END; J.mark[END] = 0u; return; }
    FwCand C{END, END, 0, kFxNoOffence, false};
    if (J.first[i] == 0x40) C = fw_candidate(J, i);
    J.nxt[0][i] = C.nxt; J.plus_of[i] = C.plus_of; J.seqlen[i] = C.off == kFxNoOffence ? C.L : 0; J.off[i] = C.off;
    J.mark[i] = i == 0 ? 1u : 0u;
}

__global__ __launch_bounds__(kFxThreads) void k_fw_jump(const FwJob J, const uint32_t round)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    if (i > J.n_lines) return;
    const uint32_t *in = J.nxt[round & 1u];
    uint32_t *out = J.nxt[(round & 1u) ^ 1u];
    uint32_t a = in[i];
    if (a > J.n_lines) a = J.n_lines;
    if (i < J.n_lines && J.mark[i]) J.mark[a] = 1u;     // (END's mark is nobody's)
    out[i] = in[a];
}

// ---- the cut of a group's files load (fastx_scan.h: the record starts of a wrapped file are the ones reachable from line 0) ----
// The job is a PIECE [a, b) of a file and a margin behind it, positions counted from a; K.b: where the piece ends.
//   k_fw_cut_next    k_fw_next's rule per candidate, as a chain to where it leaves the piece.  TERMINALS point at themselves: a
//                    line at or beyond K.b (LANDED; so is END, reached only at the file's end: "no further record" lands on n),
//                    a candidate whose outcome is open while the staged bytes are not the file's last (UNRESOLVED), a candidate
//                    that offends (OFFENCE, with its word), and what is no candidate — the fragment in front of the piece's
//                    first line start, a line of another first byte (NONE: nobody arrives there)
//   k_fw_cut_jump    k_fw_jump without marks: out[i] = in[in[i]], terminals are fixed points; after ceil(log2(lines)) + 1
//                    rounds every line holds its terminal
//   k_fw_cut_lookup  one text position: its line by bisection in pos[], that line's terminal: kind, position, offence word
__global__ __launch_bounds__(kFxThreads) void k_fw_cut_next(const FwJob J, const FwCut K)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    const uint32_t END = J.n_lines;
    if (i64 > END) return;
    const uint32_t i = (uint32_t)i64;
    uint32_t nxt = i, kind = FW_CUT_NONE;
    uint64_t off = kFxNoOffence;
    if (i == END || J.pos[i] >= K.b) kind = FW_CUT_LANDED;
    else if (i >= K.first_cand && J.first[i] == 0x40) {
        const FwCand C = fw_candidate(J, i);
        if (C.open && !K.at_eof) kind = FW_CUT_UNRESOLVED;
        else if (C.off != kFxNoOffence) { kind = FW_CUT_OFFENCE; off = C.off; }
        else { kind = FW_CUT_PASS; nxt = C.nxt; }
    }
    J.nxt[0][i] = nxt; J.mark[i] = kind; J.off[i] = off;
}

__global__ __launch_bounds__(kFxThreads) void k_fw_cut_jump(const FwJob J, const uint32_t round)
{
    const uint64_t i = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    if (i > J.n_lines) return;
    const uint32_t *in = J.nxt[round & 1u];
    uint32_t a = in[i];
    if (a > J.n_lines) a = J.n_lines;
    uint32_t t = in[a];
    if (t > J.n_lines) t = J.n_lines;
    J.nxt[(round & 1u) ^ 1u][i] = t;
}

__global__ __launch_bounds__(64) void k_fw_cut_lookup(const FwJob J, const uint32_t which, const uint64_t p, uint64_t *out)
{
    if (blockIdx.x || threadIdx.x) return;
    uint32_t lo = 0, hi = J.n_lines;                    // the first line at or behind p
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (J.pos[mid] >= p) hi = mid; else lo = mid + 1u;
    }
    uint64_t kind = FW_CUT_NONE, at = kFxNone, off = kFxNoOffence;
    if (lo < J.n_lines && J.pos[lo] == p) {
        uint32_t t = J.nxt[which & 1u][lo];
        if (t > J.n_lines) t = J.n_lines;
        kind = J.mark[t]; at = J.pos[t]; off = J.off[t];
    }
    out[0] = kind; out[1] = at; out[2] = off;
}

static constexpr int kFwWaves = kFxThreads / 64;
static constexpr uint32_t kFwRankItems = kFwRankTile / kFxThreads;

__global__ __launch_bounds__(kFxThreads) void k_fw_rank_tiles(const FwJob J)
{
    __shared__ uint64_t sh[kFwWaves];
    const uint64_t k0 = (uint64_t)blockIdx.x * kFwRankTile + (uint64_t)threadIdx.x * kFwRankItems;
    uint64_t cnt = 0, len = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFwRankItems; j++) if (k0 + j < J.n_lines && J.mark[k0 + j]) { cnt++; len += J.seqlen[k0 + j]; }
    const uint64_t t_cnt = fx_block_sum64<kFwWaves>(cnt, sh), t_len = fx_block_sum64<kFwWaves>(len, sh);
    if (threadIdx.x == 0) { J.tile_cnt[blockIdx.x] = t_cnt; J.tile_len[blockIdx.x] = t_len; }
}

__global__ __launch_bounds__(kFxThreads) void k_fw_rank_top(const FwJob J, const uint64_t n_tiles)
{
    __shared__ uint64_t sh[kFwWaves];
    const uint64_t c_cnt = fx_top_scan64<kFwWaves, FxAdd64, false>(J.tile_cnt, n_tiles, sh);
    const uint64_t c_len = fx_top_scan64<kFwWaves, FxAdd64, false>(J.tile_len, n_tiles, sh);
    if (threadIdx.x == 0) { J.tile_cnt[n_tiles] = c_cnt; J.tile_len[n_tiles] = c_len; J.tot[5] = c_cnt; J.tot[6] = c_len; }
}

__global__ __launch_bounds__(kFxThreads) void k_fw_rank_apply(const FwJob J)
{
    __shared__ uint64_t sh[kFwWaves];
    const uint64_t k0 = (uint64_t)blockIdx.x * kFwRankTile + (uint64_t)threadIdx.x * kFwRankItems;
    uint32_t m[kFwRankItems];
    uint64_t l[kFwRankItems], cnt = 0, len = 0, off = kFxNoOffence;
#pragma unroll
    for (uint32_t j = 0; j < kFwRankItems; j++) {
        m[j] = k0 + j < J.n_lines && J.mark[k0 + j] ? 1u : 0u;
        l[j] = m[j] ? J.seqlen[k0 + j] : 0;
        cnt += m[j]; len += l[j];
        if (m[j] && J.off[k0 + j] < off) off = J.off[k0 + j];
    }
    uint64_t total;
    uint64_t at = J.tile_cnt[blockIdx.x] + fx_block_prefix64<kFwWaves, FxAdd64>(cnt, sh, &total);
    uint64_t pre = J.tile_len[blockIdx.x] + fx_block_prefix64<kFwWaves, FxAdd64>(len, sh, &total);
#pragma unroll
    for (uint32_t j = 0; j < kFwRankItems; j++) {
        if (k0 + j >= J.n_lines) break;
        J.rank[k0 + j] = (uint32_t)at; J.seqpre[k0 + j] = pre;
        if (m[j]) { if (at < J.n_lines) J.hdr[at] = (uint32_t)(k0 + j); at++; pre += l[j]; }
    }
    if (off != kFxNoOffence) atomicMin(reinterpret_cast<unsigned long long *>(J.tot + 7), (unsigned long long)off);
}

__global__ __launch_bounds__(kFxThreads) void k_fw_place(const FwJob J)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kFxThreads + threadIdx.x;
    if (i64 >= J.n_lines || J.n_reads == 0 || J.n_reads > J.n_lines) return;
    const uint32_t i = (uint32_t)i64;
    if (J.mark[i]) {
        const uint64_t r = J.rank[i];
        if (r < J.n_reads) { J.rec_pos[J.read_base + r] = J.arena_base + J.pos[i]; J.seq_off[J.read_base + r] = J.text_base + J.seqpre[i]; }
    }
    uint64_t a = 0, b = J.n_reads - 1;                  // the last record whose header line is at or in front of line i (record 0's is line 0)
    while (a < b) {
        const uint64_t mid = (a + b + 1) >> 1;
        if (J.hdr[mid] <= i) a = mid; else b = mid - 1;
    }
    const uint32_t h = J.hdr[a];
    uint64_t delta = kFxNone;
    if (h < J.n_lines && i > h && i < J.plus_of[h]) delta = J.text_base + J.seqpre[h] + (J.G[i] - J.G[h + 1u]);
    J.delta[i] = delta;
}

__global__ __launch_bounds__(kFxThreads) void k_fw_emit(const FwJob J)
{
    __shared__ uint32_t s_w[kFxThreads / 64];
    const uint64_t q0 = (uint64_t)blockIdx.x * kFxTileBytes + 16u * threadIdx.x;
    const FwBase B = J.base[blockIdx.x];
    FxVec V;
    fx_load(fw_as_fx(J), q0, V);
    uint32_t tot;
    const uint32_t a = fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.ls), s_w, &tot);
    const uint32_t b = fx_scan_add<kFxThreads / 64>((uint32_t)__builtin_popcount(V.gr), s_w, &tot);
    uint64_t line = B.ls + a - 1u;                      // the line that reaches into the vector (wraps to -1 in front of line 0: no valid byte is there)
    uint64_t g = B.g + b;                               // bytes 33..126 in front of the vector
    uint32_t rem = V.ls, lo = 0;
    for (;;) {                                          // the bytes [lo, hi) of one line: the one that reaches in, then every one that starts here
        const uint32_t hi = rem ? (uint32_t)__builtin_ctz(rem) : 16u;
        uint32_t gm = V.gr & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        if (gm) {
            const uint64_t d = line < J.n_lines ? J.delta[line] : kFxNone;
            const uint64_t g_line = d != kFxNone ? J.G[line] : 0;      // (bytes 33..126 in front of the line)
            if (d == kFxNone) g += (uint32_t)__builtin_popcount(gm);
            else for (; gm; gm &= gm - 1u, g++) {
                const uint32_t j = (uint32_t)__builtin_ctz(gm);
                const uint64_t at = d + (g - g_line);
                if (at >= J.text_base && at < J.text_cap) J.text[at] = (uint8_t)(V.w[j >> 2] >> (8 * (j & 3)));
            }
        }
        if (!rem) break;
        lo = hi; rem &= rem - 1u; line++;
    }
}

// ---- host: the scratch and the launches ----
static uint64_t fw_words(uint64_t bytes) { return (bytes + 7) / 8; }

uint64_t fw_scratch_words(uint64_t n_tiles, uint64_t n_lines)
{
    const uint64_t n1 = n_lines + 1, rt = (n_lines + kFwRankTile - 1) / kFwRankTile + 1;
    return kFwTot + fw_words(n_tiles * sizeof(FwTile)) + fw_words(n_tiles * sizeof(FwBase)) + 4 * n1 /* pos G D F */ + 4 * n1 /* seqlen off seqpre delta */ +
           2 * rt + 7 * fw_words(4 * n1) /* plus nxt[2] mark plus_of rank hdr */ + fw_words(n1);
}

void fw_lay_out(FwJob &J, uint64_t *p)
{
    const uint64_t n1 = (uint64_t)J.n_lines + 1, rt = ((uint64_t)J.n_lines + kFwRankTile - 1) / kFwRankTile + 1;
    auto take = [&](uint64_t words) { uint64_t *q = p; p += words; return q; };
    J.tot = take(kFwTot);
    J.base = reinterpret_cast<FwBase *>(take(fw_words(J.n_tiles * sizeof(FwBase))));
    J.tiles = reinterpret_cast<FwTile *>(take(fw_words(J.n_tiles * sizeof(FwTile))));
    J.pos = take(n1); J.G = take(n1); J.D = take(n1); J.F = take(n1);
    J.seqlen = take(n1); J.off = take(n1); J.seqpre = take(n1); J.delta = take(n1);
    J.tile_cnt = take(rt); J.tile_len = take(rt);
    uint32_t **w32[] = {&J.plus, &J.nxt[0], &J.nxt[1], &J.mark, &J.plus_of, &J.rank, &J.hdr};
    for (uint32_t **w : w32) *w = reinterpret_cast<uint32_t *>(take(fw_words(4 * n1)));
    J.first = reinterpret_cast<uint8_t *>(take(fw_words(n1)));
}

hipError_t launch_fw_tiles(const FwJob &J, hipStream_t st)
{
    if (!J.n || !J.n_tiles || J.n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_fw_summary, dim3((unsigned)J.n_tiles), dim3(kFxThreads), 0, st, J);
    CRASS_LAUNCH(k_fw_tile_scan, dim3(1), dim3(kFxScanThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_fw_analyse(const FwJob &J, hipStream_t st)
{
    if (!J.n_lines || J.n_lines == 0xFFFFFFFFu || !J.n_tiles || J.n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const unsigned line_blocks = (unsigned)(((uint64_t)J.n_lines + 1 + kFxThreads - 1) / kFxThreads);
    const uint64_t rank_tiles = ((uint64_t)J.n_lines + kFwRankTile - 1) / kFwRankTile;
    CRASS_LAUNCH(k_fw_lines, dim3((unsigned)J.n_tiles), dim3(kFxThreads), 0, st, J);
    CRASS_LAUNCH(k_fw_next, dim3(line_blocks), dim3(kFxThreads), 0, st, J);
    uint32_t rounds = 1;                                // ceil(log2(lines)) + 1: every line could be a record
    while (rounds <= 32 && (1ull << (rounds - 1)) < J.n_lines) rounds++;
    for (uint32_t k = 0; k < rounds; k++) CRASS_LAUNCH(k_fw_jump, dim3(line_blocks), dim3(kFxThreads), 0, st, J, k);
    CRASS_LAUNCH(k_fw_rank_tiles, dim3((unsigned)rank_tiles), dim3(kFxThreads), 0, st, J);
    CRASS_LAUNCH(k_fw_rank_top, dim3(1), dim3(kFxThreads), 0, st, J, rank_tiles);
    CRASS_LAUNCH(k_fw_rank_apply, dim3((unsigned)rank_tiles), dim3(kFxThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_fw_cut(const FwJob &J, const FwCut &K, hipStream_t st, uint32_t *which)
{
    if (!J.n_lines || J.n_lines == 0xFFFFFFFFu || !J.n_tiles || J.n_tiles > 0x7FFFFFFFull || !which) return hipErrorInvalidValue;
    const unsigned line_blocks = (unsigned)(((uint64_t)J.n_lines + 1 + kFxThreads - 1) / kFxThreads);
    CRASS_LAUNCH(k_fw_lines, dim3((unsigned)J.n_tiles), dim3(kFxThreads), 0, st, J);
    CRASS_LAUNCH(k_fw_cut_next, dim3(line_blocks), dim3(kFxThreads), 0, st, J, K);
    uint32_t rounds = 1;                                // ceil(log2(lines)) + 1, as launch_fw_analyse's
    while (rounds <= 32 && (1ull << (rounds - 1)) < J.n_lines) rounds++;
    for (uint32_t k = 0; k < rounds; k++) CRASS_LAUNCH(k_fw_cut_jump, dim3(line_blocks), dim3(kFxThreads), 0, st, J, k);
    *which = rounds & 1u;                               // (round k writes nxt[(k & 1) ^ 1])
    return hipGetLastError();
}

hipError_t launch_fw_cut_lookup(const FwJob &J, uint32_t which, uint64_t p, uint64_t *d_out, hipStream_t st)
{
    if (!J.n_lines || !d_out) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_fw_cut_lookup, dim3(1), dim3(64), 0, st, J, which, p, d_out);
    return hipGetLastError();
}

hipError_t launch_fw_emit(const FwJob &J, hipStream_t st)
{
    if (!J.n_lines || !J.n_tiles || J.n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const unsigned line_blocks = (unsigned)(((uint64_t)J.n_lines + kFxThreads - 1) / kFxThreads);
    CRASS_LAUNCH(k_fw_place, dim3(line_blocks), dim3(kFxThreads), 0, st, J);
    CRASS_LAUNCH(k_fw_emit, dim3((unsigned)J.n_tiles), dim3(kFxThreads), 0, st, J);
    return hipGetLastError();
}

} // namespace crass
