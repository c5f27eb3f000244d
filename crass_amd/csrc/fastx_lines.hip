// fastx_lines.hip — bytes out for listed records of a FASTA / FASTQ file's raw bytes on the device, for a caller whose bytes
// exist only in HBM: names, header lines (RH_Header / RH_Comment), quality strings (RH_Qual) and the comment kseq hands on.  All
// four have one shape: a MEASURE kernel, a lane per listed record, gives every entry's length; the lengths' prefix sum gives the
// offsets; a COPY kernel driven by the OUTPUT, a lane per byte, finds its entry in the offsets (fx_span_of) and stores nothing
// outside [out, out + total).  None is hot: about one read in a hundred is handed on.  How the bytes are read: fastx_walk.h.
//
// names of a kept table's records (crass_hip_fastx_names_of_device) — k_nm_measure_idx walks the name of record idx[k]; the prefix
// sum stays on the device, three launches and no block waiting for another: k_nm_scan_tiles sums kNmTile lengths per block,
// k_nm_scan_top turns the tile sums into the bytes in front of every tile (fx_top_scan64, the total behind the last),
// k_nm_scan_apply writes every entry's offset and off[n]; k_nm_copy reads the offsets and the records' numbers from the device.
//
// header lines — k_hl_measure: the bytes up to the '\n' (or the input's end) and the name's length, from one walk.  The host sums
// the lengths.  k_span_copy: out[i] = bytes[start[a] + i - off[a]].
//
// quality strings — k_ql_measure: a record whose header character is '@' has its quality on its fourth line, found by three line
// ends from the header character and bounded by the next record's header character: the string is the bytes 33..126 of that
// line, as kseq keeps them (a '\r' in front of the '\n' is none).  A '>' record has none.  k_qw_measure: the same by the wrapped
// rule.  k_ql_copy: where the line's first bytes are the string (every line but one with blanks inside) the byte is at
// start + k, else the lane walks the line to its k-th such byte.  No byte outside [src, min(lim, n_bytes)) of a record is read.
//
// handed comments (RH_Comment as kseq hands it on, fastx_scan.h) — build: k_cm_bits, a lane per record walks its name,
// fx_own_comment decides, the wave's ballot is one word of the own-comment bitmap; k_cm_tiles, a wave per tile of kFxCmTile
// records: the tile's last own-comment record and their number; k_cm_top, one block: the running maximum over the tiles (the
// carries) and the total.  Three launches, no block waits for another, no atomics.  fetch: k_cm_source, a lane per listed record:
// fx_comment_handed_from, the statements the host runs; the host turns the sources into positions (it keeps the record
// positions, the device does not); k_cm_measure walks the source's name and comment, k_span_copy copies from the comments' starts.
#include "fastx_walk.h"
#include "fastx_vec.h"
#include "fastx_scan.h"

namespace crass {

static constexpr int kNmWaves = kNmThreads / 64;

// the last of the n >= 1 entries whose offset is <= i (off is not decreasing, off[0] = 0: empty entries in front of it share the
// offset, so the one found is the entry that holds byte i)
static __device__ __forceinline__ uint64_t fx_span_of(const uint64_t *off, uint64_t n, uint64_t i)
{
    uint64_t a = 0, b = n - 1;
    while (a < b) {
        const uint64_t mid = (a + b + 1) >> 1;
        if (off[mid] <= i) a = mid; else b = mid - 1;
    }
    return a;
}

__global__ __launch_bounds__(kNmThreads) void k_span_copy(const SpanCopyJob J)
{
    const uint64_t i = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (i >= J.total) return;
    const uint64_t a = fx_span_of(J.off, J.n, i);
    const uint64_t p = J.start[a] + (i - J.off[a]);
    if (p < J.n_bytes) J.out[i] = J.bytes[p];
}

// ---- names ----
static constexpr uint32_t kNmTileItems = 4;                             // lengths per lane
static constexpr uint32_t kNmTile = kNmThreads * kNmTileItems;          // ... per block

__global__ __launch_bounds__(kNmThreads) void k_nm_measure_idx(const NmOfJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t g = J.idx[k];
    if (g < J.idx_base || g - J.idx_base >= J.n_reads) { *J.flag = 1u; J.len[k] = 0u; return; }
    J.len[k] = nm_len32(nm_walk<false>((uintptr_t)J.bytes, J.n_bytes, J.rec_pos[g - J.idx_base] + 1).name);      // (rec_pos < n_bytes: the insert saw every one)
}

__global__ __launch_bounds__(kNmThreads) void k_nm_scan_tiles(const NmOfJob J)
{
    __shared__ uint64_t sh[kNmWaves];
    const uint64_t k0 = (uint64_t)blockIdx.x * kNmTile + (uint64_t)threadIdx.x * kNmTileItems;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kNmTileItems; j++) if (k0 + j < J.n) v += J.len[k0 + j];
    const uint64_t s = fx_block_sum64<kNmWaves>(v, sh);
    if (threadIdx.x == 0) J.tile_sum[blockIdx.x] = s;
}

__global__ __launch_bounds__(kNmThreads) void k_nm_scan_top(const NmOfJob J, const uint64_t n_tiles)
{
    __shared__ uint64_t sh[kNmWaves];
    const uint64_t total = fx_top_scan64<kNmWaves, FxAdd64, false>(J.tile_sum, n_tiles, sh);
    if (threadIdx.x == 0) J.tile_sum[n_tiles] = total;
}

__global__ __launch_bounds__(kNmThreads) void k_nm_scan_apply(const NmOfJob J, const uint64_t n_tiles)
{
    __shared__ uint64_t sh[kNmWaves];
    const uint64_t k0 = (uint64_t)blockIdx.x * kNmTile + (uint64_t)threadIdx.x * kNmTileItems;
    uint32_t l[kNmTileItems];
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kNmTileItems; j++) { l[j] = k0 + j < J.n ? J.len[k0 + j] : 0u; v += l[j]; }
    uint64_t total;
    uint64_t at = J.tile_sum[blockIdx.x] + fx_block_prefix64<kNmWaves, FxAdd64>(v, sh, &total);
#pragma unroll
    for (uint32_t j = 0; j < kNmTileItems; j++) { if (k0 + j < J.n) J.off[k0 + j] = at; at += l[j]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) J.off[J.n] = J.tile_sum[n_tiles];
}

__global__ __launch_bounds__(kNmThreads) void k_nm_copy(const NmOfJob J)
{
    const uint64_t i = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (i >= J.limit) return;
    const uint64_t a = fx_span_of(J.off, J.n, i);
    const uint64_t r = J.idx[a] - J.idx_base;           // (an entry out of range has no byte: the bisection never ends on one ...)
    if (r >= J.n_reads) return;                         // (... and this keeps a wrong offset array from reading rec_pos out of bounds)
    const uint64_t p = J.rec_pos[r] + 1 + (i - J.off[a]);
    if (p < J.n_bytes) J.out[i] = J.bytes[p];
}

// ---- header lines ----
__global__ __launch_bounds__(kNmThreads) void k_hl_measure(const HlJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const NmSpan s = nm_walk<true>((uintptr_t)J.bytes, J.n_bytes, J.src[k]);
    J.line_len[k] = nm_len32(s.line);
    J.name_len[k] = nm_len32(s.name);
}

// ---- quality strings ----
static __device__ __forceinline__ bool ql_is_graph(uint8_t b) { return b >= 33 && b <= 126; }

__global__ __launch_bounds__(kNmThreads) void k_ql_measure(const QlJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t p0 = J.src[k];
    const uint64_t end = J.lim[k] < J.n_bytes ? J.lim[k] : J.n_bytes;
    uint64_t start = p0;
    uint32_t len = 0, flags = 0;
    if (p0 < end && J.bytes[p0] == 0x40) {
        flags = 1u;
        uint64_t p = p0;
        for (uint32_t lines = 0; lines < 3 && p < end; p++) lines += J.bytes[p] == 0x0A ? 1u : 0u;      // behind the third line end
        start = p;
        bool gap = false, dense = true;
        for (; p < end; p++) {
            const uint8_t b = J.bytes[p];
            if (b == 0x0A) break;
            if (ql_is_graph(b)) { if (gap) dense = false; if (len != 0xFFFFFFFFu) len++; }
            else gap = true;
        }
        if (dense) flags |= 2u;
    }
    J.start[k] = start; J.len[k] = len; J.flags[k] = flags;
}

// the same for a record of the wrapped class (fastx_scan.h): behind the header line the sequence lines up to the first line that
// starts with '+', L their bytes 33..126; the quality is the first L bytes 33..126 behind the '+' line, over however many lines.
// On a four-line record the answer is k_ql_measure's.
__global__ __launch_bounds__(kNmThreads) void k_qw_measure(const QlJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t p0 = J.src[k];
    const uint64_t end = J.lim[k] < J.n_bytes ? J.lim[k] : J.n_bytes;
    uint64_t start = p0;
    uint32_t len = 0, flags = 0;
    if (p0 < end && J.bytes[p0] == 0x40) {
        flags = 1u;
        uint64_t p = p0, L = 0;
        while (p < end && J.bytes[p] != 0x0A) p++;      // the header line
        p++;
        while (p < end && J.bytes[p] != 0x2B) {         // sequence lines
            for (; p < end && J.bytes[p] != 0x0A; p++) L += ql_is_graph(J.bytes[p]) ? 1u : 0u;
            p++;
        }
        while (p < end && J.bytes[p] != 0x0A) p++;      // the '+' line
        p++;
        start = p < end ? p : end;
        bool gap = false, dense = true;
        for (p = start; p < end && len < L && len != 0xFFFFFFFFu; p++) {
            if (ql_is_graph(J.bytes[p])) { if (gap) dense = false; len++; }
            else gap = true;
        }
        if (dense) flags |= 2u;
    }
    J.start[k] = start; J.len[k] = len; J.flags[k] = flags;
}

// wrapped records too (k_qw_measure): the walk to the k-th byte 33..126 goes over line ends up to the record's end
__global__ __launch_bounds__(kNmThreads) void k_ql_copy(const QlJob J)
{
    const uint64_t i = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (i >= J.total) return;
    const uint64_t a = fx_span_of(J.off, J.n, i);
    const uint64_t k = i - J.off[a];
    const uint64_t end = J.lim[a] < J.n_bytes ? J.lim[a] : J.n_bytes;
    uint64_t p = J.start[a];
    if (J.flags[a] & 2u) p += k;
    else {                                              // the line's k-th byte in 33..126
        uint64_t seen = 0;
        for (; p < end; p++) if (ql_is_graph(J.bytes[p]) && seen++ == k) break;
    }
    if (p < end) J.out[i] = J.bytes[p];
}

// ---- the comment kseq hands on (fastx_scan.h: fx_own_comment, fx_comment_handed_from) ----
// where the name that starts at pos ends: the position of its first isspace() byte, or n_bytes (pos <= n_bytes)
static __device__ __forceinline__ uint64_t cm_name_end(uintptr_t lo, uint64_t n_bytes, uint64_t pos) { return pos + nm_walk<false>(lo, n_bytes, pos).name; }

__global__ __launch_bounds__(kNmThreads) void k_cm_bits(const CmBuildJob J)
{
    const uint64_t r = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;      // (no lane leaves: the wave's 64 records are one word)
    bool own = false;
    if (r < J.n_reads) {
        const uint64_t pos = J.rec_pos[r];
        if (pos >= J.n_bytes) *J.flag = 1u;
        else {
            const uint64_t e = cm_name_end((uintptr_t)J.bytes, J.n_bytes, pos + 1);
            own = fx_own_comment(e, J.n_bytes, e < J.n_bytes ? J.bytes[e] : (uint8_t)0);
        }
    }
    const unsigned long long m = __ballot(own);
    if ((threadIdx.x & 63u) == 0 && r < J.n_reads) J.bits[r >> 6] = m;
}

// a wave per tile, a bitmap word per lane: 1 + the tile's last own-comment record (0: none) and how many it has
__global__ __launch_bounds__(kNmThreads) void k_cm_tiles(const CmBuildJob J, const uint64_t n_words, const uint64_t n_tiles)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * kNmWaves + (threadIdx.x >> 6);
    if (t >= n_tiles) return;                           // (the whole wave)
    const uint64_t wi = t * (kFxCmTile / 64) + lane;
    const uint64_t v = wi < n_words ? J.bits[wi] : 0ull;
    const uint64_t last = fx_wave_all64<FxMax64>(v ? wi * 64 + (63u - (uint32_t)__builtin_clzll(v)) + 1 : 0ull);
    const uint64_t cnt = fx_wave_sum64((uint64_t)__builtin_popcountll(v));
    if (lane == 0) { J.carry[t] = last; J.tile_cnt[t] = cnt; }
}

// one block: carry[t] becomes the maximum over the tiles up to and including t, tile_cnt[n_tiles] the total
__global__ __launch_bounds__(kNmThreads) void k_cm_top(const CmBuildJob J, const uint64_t n_tiles)
{
    __shared__ uint64_t sh[kNmWaves];
    (void)fx_top_scan64<kNmWaves, FxMax64, true>(J.carry, n_tiles, sh);
    uint64_t cnt = 0;
    for (uint64_t t = threadIdx.x; t < n_tiles; t += kNmThreads) cnt += J.tile_cnt[t];
    const uint64_t total = fx_block_sum64<kNmWaves>(cnt, sh);
    if (threadIdx.x == 0) J.tile_cnt[n_tiles] = total;
}

__global__ __launch_bounds__(kNmThreads) void k_cm_source(const CmFetchJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t r = J.idx[k];
    J.src[k] = r < J.n_reads ? fx_comment_handed_from(J.bits, J.carry, J.file_read_base, J.n_files, r) : kFxNone;
}

// pos[k]: the first byte behind the header character of entry k's source, kFxNone where nothing is handed
__global__ __launch_bounds__(kNmThreads) void k_cm_measure(const CmFetchJob J)
{
    const uint64_t k = (uint64_t)blockIdx.x * kNmThreads + threadIdx.x;
    if (k >= J.n) return;
    const uint64_t pos = J.pos[k];
    uint64_t start = 0, line = 0;
    if (pos <= J.n_bytes) {                             // (kFxNone is beyond every input)
        const uintptr_t lo = (uintptr_t)J.bytes;
        const uint64_t e = cm_name_end(lo, J.n_bytes, pos);
        if (fx_own_comment(e, J.n_bytes, e < J.n_bytes ? J.bytes[e] : (uint8_t)0)) {      // (so for every source: its bit says so)
            start = e + 1;
            line = nm_walk<true>(lo, J.n_bytes, start).line;
        }
    }
    J.start[k] = start;
    J.len[k] = nm_len32(line);
}

// ---- host: the launches, each behind its own checks ----
uint32_t nm_scan_tile() { return kNmTile; }

hipError_t launch_span_copy(const SpanCopyJob &J, hipStream_t st)
{
    if (!J.n) return hipErrorInvalidValue;
    return NM_LAUNCH(k_span_copy, J.total, kNmThreads, st, J);
}

hipError_t launch_nm_measure_idx(const NmOfJob &J, hipStream_t st) { return NM_LAUNCH(k_nm_measure_idx, J.n, kNmThreads, st, J); }

hipError_t launch_nm_scan(const NmOfJob &J, hipStream_t st)
{
    unsigned g;
    if (!nm_grid(J.n, kNmTile, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_nm_scan_tiles, dim3(g), dim3(kNmThreads), 0, st, J);
    CRASS_LAUNCH(k_nm_scan_top, dim3(1), dim3(kNmThreads), 0, st, J, (uint64_t)g);
    CRASS_LAUNCH(k_nm_scan_apply, dim3(g), dim3(kNmThreads), 0, st, J, (uint64_t)g);
    return hipGetLastError();
}

hipError_t launch_nm_copy(const NmOfJob &J, hipStream_t st)
{
    if (!J.n) return hipErrorInvalidValue;
    return NM_LAUNCH(k_nm_copy, J.limit, kNmThreads, st, J);
}

hipError_t launch_hl_measure(const HlJob &J, hipStream_t st) { return NM_LAUNCH(k_hl_measure, J.n, kNmThreads, st, J); }
hipError_t launch_ql_measure(const QlJob &J, hipStream_t st) { return NM_LAUNCH(k_ql_measure, J.n, kNmThreads, st, J); }
hipError_t launch_qw_measure(const QlJob &J, hipStream_t st) { return NM_LAUNCH(k_qw_measure, J.n, kNmThreads, st, J); }

hipError_t launch_ql_copy(const QlJob &J, hipStream_t st)
{
    if (!J.n) return hipErrorInvalidValue;
    return NM_LAUNCH(k_ql_copy, J.total, kNmThreads, st, J);
}

hipError_t launch_cm_build(const CmBuildJob &J, hipStream_t st)
{
    unsigned g, gt;
    const uint64_t n_words = (J.n_reads + 63) / 64, n_tiles = (J.n_reads + kFxCmTile - 1) / kFxCmTile;
    if (!nm_grid(J.n_reads, kNmThreads, &g) || !nm_grid(n_tiles, kNmWaves, &gt) || !J.bits || !J.carry || !J.tile_cnt || !J.flag) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_cm_bits, dim3(g), dim3(kNmThreads), 0, st, J);
    CRASS_LAUNCH(k_cm_tiles, dim3(gt), dim3(kNmThreads), 0, st, J, n_words, n_tiles);
    CRASS_LAUNCH(k_cm_top, dim3(1), dim3(kNmThreads), 0, st, J, n_tiles);
    return hipGetLastError();
}

hipError_t launch_cm_source(const CmFetchJob &J, hipStream_t st)
{
    if (!J.n_files || !J.n_reads) return hipErrorInvalidValue;
    return NM_LAUNCH(k_cm_source, J.n, kNmThreads, st, J);
}

hipError_t launch_cm_measure(const CmFetchJob &J, hipStream_t st) { return NM_LAUNCH(k_cm_measure, J.n, kNmThreads, st, J); }

} // namespace crass
