// kernels.hip — hand-written HIP kernels for gfx950 (MI355X, CDNA4, wave64): pass 1's seed filter and position hints.
//
// The hot path of crass's WorkHorse search (reference citations are relative to the
// crass v1.0.1 tree):
//   pass 1  searchCore / scanRight / extendPreRepeat / qcFoundRepeats / DRLowLexi
//           (src/crass/libcrispr.cpp:170-395,520-1069, ReadHolder.cpp:513-609,
//            PatternMatcher.cpp:26-204)
//             the seed-scan filters and the per-position seed hints                 this file
//             searchCore for a survivor, one wave per read; Levenshtein batch       survivor_wave.hip
//             long reads' light walk                                                long_light.hip
//             searchCore for a survivor, one read per lane                          survivor_lanes.hip
//             (those three are one translation unit, survivors.hip)
//             the bit helpers these share, each defined once                        search_bits.h
//   pass 2  findSingletons / on_match over an Aho-Corasick automaton
//           (src/crass/libcrispr.cpp:399-518, src/aho-corasick/acism.c:25-106)     pass2.hip
//   ordered compaction, de-duplication and the hand-off blobs of both passes         sinks.hip
//
// This file keeps its name: the benchmark's source hash reads kernels.hip and dmerge.hip by name, so that hash now covers the
// filter stage and the merge only — a change to the survivor kernels or the light walk does not move it.
//
// Integer/byte work, HBM- and issue-bound: no MFMA.  Reads are 2-bit packed and streamed
// once per pass; wave64 ballot/ffs gives Boyer-Moore's "leftmost occurrence" for free;
// the pass-2 automaton is staged in LDS when it fits.  Compile with -ffp-contract=off:
// qcFoundRepeats' float evaluation order is part of the parity contract.
#include "search_bits.h"

namespace crass {

// ------------------------------------------------------------------------------------
// pass 1, step 1: seed-scan filter (general parameters, any read length)
//
// Contract: bit r of hitmask is set if searchCore's seed loop (libcrispr.cpp:295-348) finds a
// w-mer hit for SOME seed j on the stride-`skips` lattice.  searchCore leaves the lattice only
// after a hit (:390), so a clear bit proves searchCore returns false.  A superset is allowed
// (survivors are re-evaluated exactly by k_survivor).
// One wave scans 64 consecutive reads (one mask word); per read the packed words are staged in
// LDS, lanes span the <=64 candidate positions of a seed window and a ballot says "found".
// ------------------------------------------------------------------------------------
#define FG_WAVES 4

__global__ __launch_bounds__(FG_WAVES * WAVE) void k_filter_general(DevReads R, DevParams P, uint64_t *hitmask,
                                                                      uint32_t lds_words_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t fg_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t *words = fg_lds + (size_t)wave * lds_words_per_wave;
    const uint64_t n_words = (R.n_reads + 63) / 64;
    const uint32_t w = P.window;
    const uint32_t cmask = (1u << (2 * w)) - 1u;
    for (uint64_t mw = blockIdx.x * (uint64_t)FG_WAVES + wave; mw < n_words; mw += (uint64_t)gridDim.x * FG_WAVES) {
        uint64_t bits = 0;
        for (int k = 0; k < 64; k++) {
            uint64_t r = mw * 64 + k;
            if (r >= R.n_reads) break;
            // exc_survive: exception reads are screened on their packed words like every other read (a non-ACGT byte
            // packs as 'A', so byte-equal seeds are code-equal: still a superset) and evaluated byte-wise afterwards
            if (!P.exc_survive && rd_is_exc(R, r)) continue;
            uint32_t L = rd_len(R, r);
            int searchEnd = (int)(L - P.lowDR - P.lowSp - w - 1);
            if (searchEnd < 0) continue;
            uint32_t nw = (L + 15) >> 4;
            const uint32_t *g = R.packed + rd_word_off(R, r);
            wave_sync();
            for (uint32_t i = lane; i < nw + 1; i += 64) words[i] = (i < nw) ? g[i] : 0u;
            wave_sync();
            bool hit = false;
            for (uint32_t j = 0; j <= (uint32_t)searchEnd && !hit; j += P.skips) {
                uint32_t begin = j + P.lowDR + P.lowSp;
                uint32_t end = j + P.highDR + P.highSp + w;
                if (end >= L) end = L - 1;
                if (end < begin) end = begin;
                uint32_t sj = lds_code(words, j, cmask);
                for (uint32_t p0 = begin; p0 + w <= end; p0 += 64) {
                    uint32_t p = p0 + lane;
                    bool ok = (p + w <= end) && (lds_code(words, p, cmask) == sj);
                    if (__ballot(ok)) { hit = true; break; }
                }
            }
            if (hit) bits |= (1ull << k);
        }
        if (lane == 0) hitmask[mw] = bits;
    }
}

hipError_t launch_filter_general(const DevReads &R, const DevParams &P, uint64_t *hitmask, uint32_t max_len, hipStream_t st)
{
    uint32_t wpw = ((max_len + 15) / 16 + 2 + 3) & ~3u;
    size_t lds = (size_t)FG_WAVES * wpw * 4;
    uint64_t n_words = (R.n_reads + 63) / 64;
    uint64_t blocks = (n_words + FG_WAVES - 1) / FG_WAVES;
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (blocks == 0) return hipSuccess;
    CRASS_LAUNCH(k_filter_general, dim3((unsigned)blocks), dim3(FG_WAVES * WAVE), lds, st, R, P, hitmask, wpw);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// pass 1, step 1 (fast path): lane-per-read bit-parallel seed scan.
// Requirements: window == 8 and skips == 8 (defaults: every lattice seed is exactly one
// aligned halfword of the packed read), uniform stride <= 16 words (reads <= 256 bp).
// For a shift d, X = R ^ (R >> 2d) has a zero halfword h  <=>  the 8-mer at seed j=8h
// re-occurs at j+d.  v_pk_min_u16 accumulates "any zero so far" per halfword over all
// shifts d in [lowDR+lowSp, highDR+highSp]; a final per-halfword test yields the hit bit.
// The window's right clamp (libcrispr.cpp:301-304) and bases in the padding are ignored:
// that can only ADD survivors (superset contract), never lose one.
// ------------------------------------------------------------------------------------

// Fully unrolled implementation: D0..D1 are compile-time so every register index is static.
// LCT: compile-time read length (0 = unknown).  With it, shifts that would put the window past the
// read end (libcrispr.cpp:301-304: p <= L-9-w... i.e. d <= L-9-16k for the seeds of word k) are dropped
// at compile time: 234 instead of 343 (word, shift) pairs at L = 150.
typedef uint32_t ff_u32x2 __attribute__((ext_vector_type(2), aligned(4)));
// The W packed words of read r (r < n_reads).
template <int W, int N>
static __device__ __forceinline__ void ff_load_words(const DevReads &R, uint64_t r, uint32_t (&w)[N])
{
    const uint32_t *g = R.packed + r * (uint64_t)W;
    // a row is dword-aligned only; global_load_dwordx4 takes that on gfx950, so W words are W/4 wide loads and a tail
#pragma unroll
    for (int i = 0; i + 4 <= W; i += 4) {
        const ff_u32x4 v = *reinterpret_cast<const ff_u32x4 *>(g + i);
        w[i] = v.x; w[i + 1] = v.y; w[i + 2] = v.z; w[i + 3] = v.w;
    }
    if ((W & 3) >= 2) {
        const ff_u32x2 v = *reinterpret_cast<const ff_u32x2 *>(g + (W & ~3));
        w[W & ~3] = v.x; w[(W & ~3) + 1] = v.y;
    }
    if (W & 1) w[W - 1] = g[W - 1];
}
// One read's row (W words, zero when r is past the end) and its exception flag.
template <int W>
static __device__ __forceinline__ void ff_load_row(const DevReads &R, const DevParams &P, uint64_t r, uint32_t (&w)[W], uint64_t &exc_word)
{
#pragma unroll
    for (int i = 0; i < W; i++) w[i] = 0;
    // the wave's 64 exception bits: one scalar load (the mask has a spare word, engine.cpp load_reads), off the vector memory
    // counter so that waiting for it does not wait for the row
    exc_word = 0;
    const uint64_t wave_word = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(r >> 38)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)(r >> 6));
    if (!P.exc_survive && (wave_word << 6) < R.n_reads) {
        const uint32_t *e = R.exc_mask + 2 * wave_word;
        exc_word = (uint64_t)e[0] | ((uint64_t)e[1] << 32);
    }
    if (r < R.n_reads) ff_load_words<W>(R, r, w);
}

// The same request for the kernels that keep the NEXT row in flight while they scan one: every load is unconditional, from a
// read index clamped to the last read (r_last = n_reads - 1), and the exception word's is only under wave-uniform conditions.
// A load under a lane predicate is a divergent branch, and behind its join the compiler's wait for the OLDER row came out as
// vmcnt(0) — it waited for the row just requested too (profiles/NOTES_r17.md).  A clamped lane's row is never used: the callers
// test r < n_reads where a result leaves the lane.
template <int W>
static __device__ __forceinline__ void ff_request_row(const DevReads &R, const DevParams &P, uint64_t r, uint64_t r_last, uint32_t (&w)[W], uint64_t &exc_word)
{
    uint64_t wave_word = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(r >> 38)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)(r >> 6));
    if (wave_word > (r_last >> 6)) wave_word = r_last >> 6;
    // (loaded whether it is used or not — exc_survive: eight bytes per wave and row: behind the join of even a wave-uniform
    // branch the wait for the row before must assume the path WITHOUT the load, and comes out one short)
    const uint32_t *e = R.exc_mask + 2 * wave_word;
    const uint64_t ew = (uint64_t)e[0] | ((uint64_t)e[1] << 32);
    exc_word = P.exc_survive ? 0ull : ew;
    ff_load_words<W>(R, r < r_last ? r : r_last, w);
}

// The scan of one row: acc[k] halfword h becomes 0 iff the 8-mer at seed 8 (2k + h) re-occurs at some shift D0 .. D1.
// (early(): called once behind the first shift, i.e. behind the wait for the row — where a streaming caller puts a store)
struct ff_nothing { __device__ __forceinline__ void operator()() const {} };
template <int D0, int D1, int LCT, int WX, int SW, typename F = ff_nothing>
static __device__ __forceinline__ void ff_exact_scan(const uint32_t (&w)[WX], uint32_t (&acc)[SW], F &&early = F())
{
#pragma unroll
    for (int i = 0; i < SW; i++) acc[i] = 0xFFFFFFFFu;
#pragma unroll
    for (int d = D0; d <= D1; d++) {
        if (d == D0 + 1) early();
        const int q = d >> 4;
        const int sh = (d & 15) * 2;
#pragma unroll
        for (int k = 0; k < SW; k++) {
            if (LCT > 0 && d > LCT - 9 - 16 * k) continue;               // window past the read end for both seeds of word k
            uint32_t lo = w[k + q], hi = w[k + q + 1];
            uint32_t s = sh ? ((lo >> sh) | (hi << (32 - sh))) : lo;      // v_alignbit_b32
            uint32_t x = s ^ w[k];
            // per-halfword running minimum: a halfword of acc becomes 0 iff some x halfword was 0
            acc[k] = pk_min_u16(acc[k], x);
        }
    }
}
// ... and its hint: bit h set iff lattice seed j = 8h may have a hit (superset); halfwords 0 .. n_seed-1 hold lattice seeds.
template <int LCT, int SW>
static __device__ __forceinline__ uint32_t ff_exact_hint(const uint32_t (&acc)[SW], int n_seed)
{
    // min(halfword, 1) is 0 exactly for a hit; the words are folded two bits apart (low halfwords -> bits 2k, high -> bits
    // 2k + 16) and the halves interleaved at the end
    uint32_t t0 = 0, t1 = 0;                        // words 0..7 and 8..15 (a fold holds 16 seeds)
#pragma unroll
    for (int k = 0; k < SW; k++) {
        if (LCT > 0 && 2 * k >= n_seed) continue;
        const uint32_t f = pk_nonzero_u16(acc[k]);
        if (k < 8) t0 |= f << (2 * k); else t1 |= f << (2 * (k - 8));
    }
    uint32_t miss = (t0 | (t0 >> 15)) & 0xFFFFu;
    if (SW > 8) miss |= (t1 | (t1 >> 15)) << 16;
    return ~miss & (n_seed >= 32 ? 0xFFFFFFFFu : ((1u << n_seed) - 1u));
}

// RPL: reads per lane.  A lane's reads are 256 apart (a wave still covers 64 consecutive reads, one mask word); the row of the
// next read is requested before the current one is scanned and the wait for the current one is COUNTED (vmcnt(4): the next
// row's three loads and its exception word stay outstanding), so a wave's only exposed memory latency is its first load.
// (Until round 17 the loads sat under the lane's r < n_reads and the waits came out as vmcnt(0): the rows were in effect
// awaited in pairs, two exposed round trips per four rows.  ff_request_row, profiles/NOTES_r17.md.)
template <int W, int D0, int D1, int LCT, int RPL>
__global__ __launch_bounds__(256) void k_filter_fast_impl(DevReads R, DevParams P, uint64_t *hitmask, uint32_t *seed_hint, uint8_t *clear_found)
{
    const uint64_t r_first = blockIdx.x * (uint64_t)(256 * RPL) + threadIdx.x;
    // the step's found flags (one byte per header id, n + 1 of them) are cleared on the way: 64 consecutive bytes per wave and row
    // beside 2.5 KB of loads, instead of a 12-100 MB fill kernel in front of every seed scan (6-30 us of the step)
    if (clear_found && r_first == 0) clear_found[R.n_reads] = 0;
    constexpr int WX = W + (D1 >> 4) + 2;
    const uint64_t r_last = R.n_reads - 1;
    uint32_t nxt[W];
    uint64_t nxt_exc;
    if constexpr (RPL > 1) ff_request_row<W>(R, P, r_first, r_last, nxt, nxt_exc);
    else ff_load_row<W>(R, P, r_first, nxt, nxt_exc);   // (one row per lane: nothing to keep in flight, the form of round 7)
#pragma unroll
    for (int it = 0; it < RPL; it++) {
    const uint64_t r = r_first + (uint64_t)it * 256u;
    const bool active = r < R.n_reads;
    if constexpr (RPL == 1) { if (clear_found && active) clear_found[r] = 0; }
    uint32_t w[WX];
#pragma unroll
    for (int i = 0; i < WX; i++) w[i] = i < W ? nxt[i] : 0u;
    const bool exc = (nxt_exc >> (r & 63)) & 1u;        // (exception reads are left to their own pass, see k_filter_general)
    if (it + 1 < RPL) {
        ff_request_row<W>(R, P, r + 256u, r_last, nxt, nxt_exc);
        __builtin_amdgcn_sched_barrier(0);              // (the requests stay IN FRONT of the scan: left alone the scheduler sinks them four fifths into it)
    }
    const uint32_t L = active ? rd_len(R, r) : 0u;
    // seeds live in halfwords 0 .. searchEnd/8 with searchEnd = L-58 <= 16W-58: only words < SW hold one
    constexpr int SW = ((16 * W - 58) / 8 + 2) / 2;
    uint32_t acc[SW];
    // (the flag's store counts on vmcnt like the loads.  Issued just behind the wait for this row — a whole scan before the next
    // wait — and by every lane, a lane past the end clearing the spare byte once more, it is long complete when the next row is
    // waited for and no divergent branch holds it; in front of this row's wait it would be one more operation of unknown
    // presence between the two rows, behind the scan the next wait would sit out most of its round trip.)
    ff_exact_scan<D0, D1, LCT>(w, acc, [&]() { if constexpr (RPL > 1) { if (clear_found) clear_found[active ? r : R.n_reads] = 0; } });
    bool hit = false;
    // a uniform-length instantiation knows the seed count at compile time (D0 = lowDR + lowSp, checked by the launcher)
    const int searchEnd = LCT > 0 ? (LCT - D0 - 8 - 1) : (int)(L - P.lowDR - P.lowSp - 8 - 1);
    if (active && !exc && searchEnd >= 0) {
        const uint32_t hint = ff_exact_hint<LCT>(acc, searchEnd / 8 + 1);
        hit = hint != 0;
        if (hit) seed_hint[r] = hint;                   // sparse: ~2 % of the lanes
    }
    uint64_t m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && active) hitmask[r >> 6] = m;
    }
}

// The same filter with two shifts folded per minimum (gfx950: v_bitop3_b32, v_pk_minimum3_f16), for uniform lengths and RPL rows.
// LOOSE scan: x = (s ^ w[k]) & 0x3FFF3FFF is one v_bitop3_b32; a halfword of it read as f16 has sign 0 and an exponent below
// all-ones (no NaN, no Inf; denormals are kept: profiles/ubench/valu_rate_asm_bitop3_mi355x.txt checks every triple), so
// v_pk_minimum3_f16 is the UNSIGNED minimum of three such words: acc = minimum3(acc, x_d, x_d+1), three instructions per two
// (word, shift) pairs instead of four.  The mask drops the seed's eighth base from the comparison: a zero halfword now means "the
// 7-mer re-occurs", which every exact hit is and ~3 % of random reads are.  EXACT recheck: loose-positive lanes queue their read
// in LDS; when the block's rows are done its waves take 64 queued reads at a time, reload their rows (L2-hot) and run
// k_filter_fast_impl's own scan, which decides the read's mask bit and hint.  hitmask and seed_hint are bit for bit
// k_filter_fast_impl's.  A wave's mask word gets its bits from rechecked reads of other lanes, so the block's 4 RPL words are
// built in LDS and stored once each at the end.
static __device__ __forceinline__ uint32_t pk_minimum3_f16(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
template <int W, int D0, int D1, int LCT, int RPL>
__global__ __launch_bounds__(256) void k_filter_fast_pairs(DevReads R, DevParams P, uint64_t *hitmask, uint32_t *seed_hint, uint8_t *clear_found)
{
    static_assert(LCT > 0 && LCT - D0 - 9 >= 0 && RPL * 256 <= 65536, "uniform length with at least one seed");
    __shared__ uint32_t q_n;
    __shared__ uint16_t q[256 * RPL];                   // reads to recheck, as offsets into the block (every lane and row at most once)
    __shared__ uint32_t tile_mask[2 * 4 * RPL];         // the block's mask words, as 32-bit halves
    const uint64_t r_block = blockIdx.x * (uint64_t)(256 * RPL);
    const uint64_t r_first = r_block + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    if (clear_found && r_first == 0) clear_found[R.n_reads] = 0;
    constexpr int WX = W + (D1 >> 4) + 2;
    constexpr int SW = ((16 * W - 58) / 8 + 2) / 2;
    constexpr int n_seed = (LCT - D0 - 9) / 8 + 1;
    constexpr uint32_t M14 = 0x3FFF3FFFu;
    const uint64_t r_last = R.n_reads - 1;
    uint32_t nxt[W];
    uint64_t nxt_exc;
    ff_request_row<W>(R, P, r_first, r_last, nxt, nxt_exc);
    if (threadIdx.x < 2 * 4 * RPL) tile_mask[threadIdx.x] = 0;
    if (threadIdx.x == 0) q_n = 0;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RPL; it++) {
        const uint64_t r = r_first + (uint64_t)it * 256u;
        const bool active = r < R.n_reads;
        uint32_t w[WX];
#pragma unroll
        for (int i = 0; i < WX; i++) w[i] = i < W ? nxt[i] : 0u;
        const bool exc = (nxt_exc >> (r & 63)) & 1u;
        if (it + 1 < RPL) {
            ff_request_row<W>(R, P, r + 256u, r_last, nxt, nxt_exc);
            __builtin_amdgcn_sched_barrier(0);          // (the requests stay IN FRONT of the scan: left alone the scheduler sinks them four fifths into it)
        }
        uint32_t acc[SW];
#pragma unroll
        for (int i = 0; i < SW; i++) acc[i] = 0x3C003C00u;
#pragma unroll
        for (int d = D0; d <= D1; d += 2) {
            // (the found flag's store, just behind the wait for this row and by every lane: see k_filter_fast_impl)
            if (d == D0 + 2 && clear_found) clear_found[active ? r : R.n_reads] = 0;
#pragma unroll
            for (int k = 0; k < SW; k++) {
                if (d > LCT - 9 - 16 * k) continue;
                const int q0 = d >> 4, sh0 = (d & 15) * 2;
                const uint32_t s0 = sh0 ? __builtin_amdgcn_alignbit(w[k + q0 + 1], w[k + q0], sh0) : w[k + q0];
                const uint32_t a = (s0 ^ w[k]) & M14;                                   // v_bitop3_b32
                uint32_t b = a;                                                         // (an odd shift left over)
                if (d + 1 <= D1 && d + 1 <= LCT - 9 - 16 * k) {
                    const int q1 = (d + 1) >> 4, sh1 = ((d + 1) & 15) * 2;
                    const uint32_t s1 = sh1 ? __builtin_amdgcn_alignbit(w[k + q1 + 1], w[k + q1], sh1) : w[k + q1];
                    b = (s1 ^ w[k]) & M14;
                }
                acc[k] = pk_minimum3_f16(acc[k], a, b);
            }
        }
        // loose-positive: some seed halfword is zero (a seedless high half of the last word may count: the recheck decides)
        uint32_t m = 0x3C003C00u;
#pragma unroll
        for (int k = 0; 2 * k < n_seed; k += 2) m = pk_minimum3_f16(m, acc[k], 2 * (k + 1) < n_seed ? acc[k + 1] : acc[k]);
        const bool pos = active && !exc && pk_nonzero_u16(m) != 0x00010001u;
        const uint64_t pm = __ballot(pos);
        if (pm) {                                                                       // (wave-uniform)
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&q_n, (uint32_t)__popcll(pm));
            base = __builtin_amdgcn_readfirstlane(base);
            const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
            if (pos) q[base + before] = (uint16_t)(it * 256 + threadIdx.x);
        }
    }
    __syncthreads();
    const uint32_t qn = q_n;
    for (uint32_t b0 = threadIdx.x & ~63u; b0 < qn; b0 += 256u) {                        // (wave-uniform)
        const bool have = b0 + lane < qn;
        const uint32_t loc = have ? q[b0 + lane] : 0u;
        uint32_t w[WX];
#pragma unroll
        for (int i = 0; i < WX; i++) w[i] = 0u;
        if (have) ff_load_words<W>(R, r_block + loc, w);
        uint32_t acc[SW];
        ff_exact_scan<D0, D1, LCT>(w, acc);
        const uint32_t hint = ff_exact_hint<LCT>(acc, n_seed);
        if (have && hint != 0) {
            seed_hint[r_block + loc] = hint;
            atomicOr(&tile_mask[loc >> 5], 1u << (loc & 31u));
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 * RPL) {
        const uint64_t r0 = r_block + threadIdx.x * 64u;
        if (r0 < R.n_reads) hitmask[r0 >> 6] = (uint64_t)tile_mask[2 * threadIdx.x] | ((uint64_t)tile_mask[2 * threadIdx.x + 1] << 32);
    }
}

// The same scan for ANY shift range (-s / -S / -D: the seed lattice and the window are the defaults', only the distances at
// which a copy counts change): D0 = lowDR + lowSp .. D1 = highDR + highSp arrive at run time.  The fixed-range kernel indexes its
// registers with compile-time shifts; here the WORD part of a shift (d >> 4) stays a compile-time loop — static register
// indices —, the sixteen bit offsets inside it are sixteen copies of the three instructions behind one scalar branch each, and a
// funnel shift takes its amount from a register as readily as from an immediate: the instructions executed are the fixed
// kernel's for the same range.  (k_filter_general, which every non-default option set took until round 5, is a wave per 64
// reads through LDS: 10.6 ms for 10 M reads with -s 20 -S 60 against 0.18 ms for the defaults.)
template <int W>
__global__ __launch_bounds__(256) void k_filter_fast_range(DevReads R, DevParams P, uint64_t *hitmask, uint32_t *seed_hint)
{
    const uint64_t r = blockIdx.x * (uint64_t)256 + threadIdx.x;
    constexpr int WX = 2 * W + 2;                       // shifts up to 16 W + 15 bases: beyond a read of this stride nothing matches
    uint32_t row[W];
    uint64_t exc_word;
    ff_load_row<W>(R, P, r, row, exc_word);
    const bool active = r < R.n_reads;
    uint32_t w[WX];
#pragma unroll
    for (int i = 0; i < WX; i++) w[i] = i < W ? row[i] : 0u;
    const bool exc = (exc_word >> (r & 63)) & 1u;
    const uint32_t L = active ? rd_len(R, r) : 0u;
    constexpr int SW = ((16 * W - 26) / 8 + 2) / 2;     // words that can hold a lattice seed for ANY bounds (searchEnd <= 16 W - 26: lowDR + lowSp >= 17)
    const int D0 = (int)(P.lowDR + P.lowSp), D1 = min((int)(P.highDR + P.highSp), 16 * W + 15);
    uint32_t acc[SW];
#pragma unroll
    for (int i = 0; i < SW; i++) acc[i] = 0xFFFFFFFFu;
    const int n_seed_max = (16 * W - D0 - 9) / 8 + 1;                   // no read of this stride has a seed beyond (wave-uniform)
#pragma unroll
    for (int q = 0; q <= W; q++) {
        if (16 * q + 15 < D0 || 16 * q > D1) continue;                  // (wave-uniform: a scalar branch)
        const int sb_lo = max(0, D0 - 16 * q), sb_hi = min(15, D1 - 16 * q);
        for (int sb = sb_lo; sb <= sb_hi; sb++) {                       // (a run-time loop: the bodies below are q x k, not q x 16 x k)
            const uint32_t sh = (uint32_t)(2 * sb);
#pragma unroll
            for (int k = 0; k < SW; k++) {
                if (2 * k >= n_seed_max) continue;
                const uint32_t lo = w[k + q], hi = w[k + q + 1];
                acc[k] = pk_min_u16(acc[k], __builtin_amdgcn_alignbit(hi, lo, sh) ^ w[k]);
            }
        }
    }
    bool hit = false;
    const int searchEnd = (int)(L - P.lowDR - P.lowSp - 8 - 1);
    if (active && !exc && searchEnd >= 0) {
        const int n_seed = searchEnd / 8 + 1;
        uint32_t t0 = 0, t1 = 0;
#pragma unroll
        for (int k = 0; k < SW; k++) {
            const uint32_t f = pk_nonzero_u16(acc[k]);
            if (k < 8) t0 |= f << (2 * k); else t1 |= f << (2 * (k - 8));
        }
        uint32_t miss = (t0 | (t0 >> 15)) & 0xFFFFu;
        if (SW > 8) miss |= (t1 | (t1 >> 15)) << 16;
        const uint32_t hint = ~miss & (n_seed >= 32 ? 0xFFFFFFFFu : ((1u << n_seed) - 1u));
        hit = hint != 0;
        if (hit) seed_hint[r] = hint;
    }
    const uint64_t m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && active) hitmask[r >> 6] = m;
}

// ... and for ANY window (6 .. 9) and seed lattice (-w, -d: skips = lowDR - (2 w - 1) is then no multiple of a halfword's eight
// bases, and a w-mer no halfword).  For a shift d, X = R xor (R >> 2d) has 2 w zero bits from bit 2p  <=>  the w-mer at p
// re-occurs at p + d: the mismatch flag of a base is the OR of its two bits, a window's flag the OR of its w bases' flags — built by
// doubling (w = 8: windows of 1, 2, 4, 8 bases; three funnel-shift + OR pairs) —, and the flags are AND-ed over the shifts: a zero
// at bit 2p of the result means "some shift matches at p".  11 instructions per word and shift instead of the halfword form's 3,
// for EVERY position at once; the lattice is a mask at the end.  (k_filter_general took 7.3 ms for 10 M reads with -w 7 and 13.7 ms
// with -d 20 -D 40, against 0.18 ms for the defaults: profiles/r05_bench_c1_params_*.json.)
template <int W>
__global__ __launch_bounds__(256) void k_filter_fast_any(DevReads R, DevParams P, uint64_t *hitmask, uint32_t *seed_hint)
{
    const uint64_t r = blockIdx.x * (uint64_t)256 + threadIdx.x;
    constexpr int WX = 2 * W + 3;
    uint32_t row[W];
    uint64_t exc_word;
    ff_load_row<W>(R, P, r, row, exc_word);
    const bool active = r < R.n_reads;
    uint32_t w[WX];
#pragma unroll
    for (int i = 0; i < WX; i++) w[i] = i < W ? row[i] : 0u;
    const bool exc = (exc_word >> (r & 63)) & 1u;
    const uint32_t L = active ? rd_len(R, r) : 0u;
    const int D0 = (int)(P.lowDR + P.lowSp), D1 = min((int)(P.highDR + P.highSp), 16 * W + 15);
    const int wn = (int)P.window;
    // the doubling steps that take a base's flag to a window's (wave-uniform): windows of c bases -> c + s, s = min(c, wn - c)
    const int s1 = min(1, wn - 1), s2 = min(2, wn - 1 - s1), s3 = min(4, wn - 1 - s1 - s2), s4 = wn - 1 - s1 - s2 - s3;      // (wn <= 9: s4 <= 1)
    uint32_t nz[W];                                      // AND over the shifts of the windows' mismatch flags (even bits)
#pragma unroll
    for (int i = 0; i < W; i++) nz[i] = 0xFFFFFFFFu;
#pragma unroll
    for (int q = 0; q <= W; q++) {
        if (16 * q + 15 < D0 || 16 * q > D1) continue;                  // (wave-uniform)
        const int sb_lo = max(0, D0 - 16 * q), sb_hi = min(15, D1 - 16 * q);
        for (int sb = sb_lo; sb <= sb_hi; sb++) {
            const uint32_t sh = (uint32_t)(2 * sb);
            uint32_t z[W + 1];
#pragma unroll
            for (int k = 0; k <= W; k++) {
                const uint32_t x = __builtin_amdgcn_alignbit(w[k + q + 1], w[k + q], sh) ^ w[k];
                z[k] = x | (x >> 1);                     // (odd bits: don't care, they stay on odd bits below)
            }
            // a window of wn bases reaches at most 8 bases = 16 bits into the next word: one word of halo is enough
#pragma unroll
            for (int k = 0; k < W; k++) z[k] |= __builtin_amdgcn_alignbit(z[k + 1], z[k], (uint32_t)(2 * s1));
            if (s2 > 0) {
                z[W] |= z[W] >> (2 * s1);
#pragma unroll
                for (int k = 0; k < W; k++) z[k] |= __builtin_amdgcn_alignbit(z[k + 1], z[k], (uint32_t)(2 * s2));
            }
            if (s3 > 0) {
                z[W] |= z[W] >> (2 * s2);
#pragma unroll
                for (int k = 0; k < W; k++) z[k] |= __builtin_amdgcn_alignbit(z[k + 1], z[k], (uint32_t)(2 * s3));
            }
            if (s4 > 0) {
                z[W] |= z[W] >> (2 * s3);
#pragma unroll
                for (int k = 0; k < W; k++) z[k] |= __builtin_amdgcn_alignbit(z[k + 1], z[k], (uint32_t)(2 * s4));
            }
#pragma unroll
            for (int k = 0; k < W; k++) nz[k] &= z[k];
        }
    }
    bool hit = false;
    const int searchEnd = (int)(L - P.lowDR - P.lowSp - P.window - 1);
    if (active && !exc && searchEnd >= 0) {
        // lattice seeds j = i * skips <= searchEnd; bit i of the hint for the first 32 of them (a superset: the zero padding and the
        // clamp of the window at the read's end are ignored, as in the halfword form)
        const uint32_t skips = P.skips;
        uint32_t hint = 0, more = 0;
        uint32_t j = 0;
        for (uint32_t i = 0; j <= (uint32_t)searchEnd; i++, j += skips) {
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < W; k++) word = (j >> 4) == (uint32_t)k ? nz[k] : word;
            const uint32_t m = ((word >> (2u * (j & 15u))) & 1u) ^ 1u;
            if (i < 32u) hint |= m << i; else more |= m;
        }
        hit = (hint | more) != 0;
        if (hit) seed_hint[r] = more ? 0xFFFFFFFFu : hint;      // (a hit beyond the 32nd seed: the hint only says "walk them all")
    }
    const uint64_t m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && active) hitmask[r >> 6] = m;
}

hipError_t launch_filter_fast(const DevReads &R, const DevParams &P, uint64_t *hitmask, uint32_t *seed_hint, hipStream_t st, uint8_t *clear_found, bool *cleared)
{
    if (cleared) *cleared = false;
    if (!R.stride_words || R.n_reads == 0) return hipErrorNotSupported;
    if (P.window != 8 || P.skips != 8) {
        // another window or seed lattice (-w, -d): the every-position form
        if (P.window < 6 || P.window > 9 || P.skips < 1 || P.lowDR + P.lowSp < 17 || P.highDR + P.highSp < P.lowDR + P.lowSp) return hipErrorNotSupported;
        const uint64_t nb = (R.n_reads + 255) / 256;
        if (nb > 0x7FFFFFFFull) return hipErrorNotSupported;
        switch (R.stride_words) {
#define FA_CASE(WW) case WW: CRASS_LAUNCH((k_filter_fast_any<WW>), dim3((unsigned)nb), dim3(256), 0, st, R, P, hitmask, seed_hint); break;
            FA_CASE(4) FA_CASE(5) FA_CASE(6) FA_CASE(7) FA_CASE(8) FA_CASE(9) FA_CASE(10)
            FA_CASE(11) FA_CASE(12) FA_CASE(13) FA_CASE(14) FA_CASE(15) FA_CASE(16)
#undef FA_CASE
            default: return hipErrorNotSupported;
        }
        return hipGetLastError();
    }
    if (P.lowDR + P.lowSp != 49 || P.highDR + P.highSp != 97) {
        // another shift range (-s / -S / -D): the run-time-range form.  (The hint word has 32 bits: reads of up to 16 words.)
        if (P.lowDR + P.lowSp < 17 || P.highDR + P.highSp < P.lowDR + P.lowSp) return hipErrorNotSupported;
        const uint64_t nb = (R.n_reads + 255) / 256;
        if (nb > 0x7FFFFFFFull) return hipErrorNotSupported;
        switch (R.stride_words) {
#define FR_CASE(WW) case WW: CRASS_LAUNCH((k_filter_fast_range<WW>), dim3((unsigned)nb), dim3(256), 0, st, R, P, hitmask, seed_hint); break;
            FR_CASE(4) FR_CASE(5) FR_CASE(6) FR_CASE(7) FR_CASE(8) FR_CASE(9) FR_CASE(10)
            FR_CASE(11) FR_CASE(12) FR_CASE(13) FR_CASE(14) FR_CASE(15) FR_CASE(16)
#undef FR_CASE
            default: return hipErrorNotSupported;
        }
        return hipGetLastError();
    }
    uint64_t blocks = (R.n_reads + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorNotSupported;
    // common uniform read lengths get the compile-time clamp and, for big sets, RPL rows per lane with the next row in flight
    // (CRASS_FF_RPL = 1 | 4 forces one form for every size: the A/B and the parity sweep of the other form)
    static const int rpl_env = getenv("CRASS_FF_RPL") ? atoi(getenv("CRASS_FF_RPL")) : 0;
    const int rpl = rpl_env ? rpl_env : (R.n_reads >= (1u << 22) ? 4 : 1);
    dim3 g((unsigned)blocks), b(256), g4((unsigned)((blocks + 3) / 4));
    // (CRASS_FF_EXACT = 1 keeps k_filter_fast_impl where k_filter_fast_pairs would run: the A/B and the parity tests of the two)
    static const bool ff_exact = getenv("CRASS_FF_EXACT") && atoi(getenv("CRASS_FF_EXACT")) != 0;
    if (cleared && clear_found) *cleared = true;            // (every path below clears the found flags)
#define FF_LEN(LL, WW) if (R.uniform_len == LL && R.stride_words == WW) { \
        if (rpl >= 4 && !ff_exact) CRASS_LAUNCH((k_filter_fast_pairs<WW, 49, 97, LL, 4>), g4, b, 0, st, R, P, hitmask, seed_hint, clear_found); \
        else if (rpl >= 4) CRASS_LAUNCH((k_filter_fast_impl<WW, 49, 97, LL, 4>), g4, b, 0, st, R, P, hitmask, seed_hint, clear_found); \
        else CRASS_LAUNCH((k_filter_fast_impl<WW, 49, 97, LL, 1>), g, b, 0, st, R, P, hitmask, seed_hint, clear_found); \
        return hipGetLastError(); }
    FF_LEN(100, 7) FF_LEN(101, 7) FF_LEN(125, 8) FF_LEN(126, 8) FF_LEN(150, 10) FF_LEN(151, 10) FF_LEN(250, 16) FF_LEN(251, 16)
#undef FF_LEN
    switch (R.stride_words) {
#define FF_CASE(WW) case WW: CRASS_LAUNCH((k_filter_fast_impl<WW, 49, 97, 0, 1>), g, b, 0, st, R, P, hitmask, seed_hint, clear_found); break;
        FF_CASE(4) FF_CASE(5) FF_CASE(6) FF_CASE(7) FF_CASE(8) FF_CASE(9) FF_CASE(10)
        FF_CASE(11) FF_CASE(12) FF_CASE(13) FF_CASE(14) FF_CASE(15) FF_CASE(16)
#undef FF_CASE
        default: if (cleared) *cleared = false; return hipErrorNotSupported;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Long reads: per-POSITION seed hints.  A 10 kbp read has ~1 250 lattice seeds and a spurious hit with p ~ 0.93, so a
// per-read filter is useless there; and after a rejected candidate the seed loop leaves the lattice (libcrispr.cpp:390) for
// another residue class mod 8.  Bit p of the read's hint bitmap clear => the 8-mer at p has no copy at p+49 .. p+97 =>
// searchCore's iteration at j = p is a no-op.  This kernel fills the bits of the lattice class (p = 8 i) for every read, one
// lane per 64 positions (4 seed words + halo); the bits of another class are computed by the walking wave itself when — and
// from where — its read's walk moves there (wave_hints_class).  A superset like the short-read filter (padding bases and the
// right clamp are ignored).  Default window / bounds only.
// ------------------------------------------------------------------------------------
// the read a hint tile (64 positions) belongs to and the tile's number inside it: largest r with hint_off[r] <= t
static __device__ __forceinline__ void hint_tile_read(const DevReads &R, const uint64_t *hint_off, const uint32_t *blk_read, uint64_t t, uint64_t n_words,
                                                      uint64_t &r, uint32_t &tile)
{
    // Reads of one length: a division (the search is 20 dependent
    // loads for 1 M reads — about three times the wave's 3.8 us of arithmetic, which six waves per SIMD only just cover)
    if (R.uniform_len) {
        const uint32_t per_read = (R.uniform_len + 63u) >> 6;
        if ((n_words >> 32) == 0) {                                     // (a 32-bit division: a fifth of the 64-bit one's instructions)
            const uint32_t t32 = (uint32_t)t, r32 = t32 / per_read;
            r = r32;
            tile = t32 - r32 * per_read;
        } else {
            r = t / per_read;
            tile = (uint32_t)(t - r * per_read);
        }
    } else if (blk_read) {
        // ragged lengths: the host noted the read of every block's first tile (blk_read[b] = read of tile 256 b); a long read
        // has dozens of tiles, so the tile's own read is a few steps further (short reads mixed in: more steps, same result)
        // (... bisected between this block's first read and the next block's: reads of a few hundred bases are fifty to a block)
        uint64_t lo = blk_read[t >> 8], hi = (uint64_t)blk_read[(t >> 8) + 1] + 1;      // invariant: hint_off[lo] <= t < hint_off[hi]
        if (hi > R.n_reads) hi = R.n_reads;
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (hint_off[mid] <= t) lo = mid; else hi = mid; }
        r = lo;
        tile = (uint32_t)(t - hint_off[r]);
    } else {
        uint64_t lo = 0, hi = R.n_reads;                                // invariant: hint_off[lo] <= t < hint_off[hi]
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (hint_off[mid] <= t) lo = mid; else hi = mid; }
        r = lo;
        tile = (uint32_t)(t - hint_off[r]);
    }
}

template <bool RANGE>
__global__ __launch_bounds__(256) void k_hint_positions(DevReads R, const uint64_t *hint_off, const uint32_t *blk_read, uint64_t t0, uint64_t n_words, uint64_t *hint_bits,
                                                        int D0, int D1, uint64_t *hitmask, uint32_t exc_survive)
{
    // (t0: a multiple of 256 — the launch covers the hint words [t0, n_words), see launch_hint_positions)
    const uint64_t t = t0 + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n_words) return;
    uint64_t r;
    uint32_t tile;
    hint_tile_read(R, hint_off, blk_read, t, n_words, r, tile);
    const uint32_t L = rd_len(R, r);
    const uint32_t nw = (L + 15) >> 4;
    const uint32_t *g = R.packed + rd_word_off(R, r) + tile * 4u;
    const uint32_t rem = nw - tile * 4u;                                 // words from this tile's first to the read's end
    uint32_t w[13];
    // 13 words: the tile's four and the halo.  A wave without a lane near its read's end (6 of 10 at 10 kbp) takes them as three
    // 16-byte loads and a word from one address — no bound per word; the last read of the set never does (nothing is read
    // past the reads' buffer)
    typedef uint32_t hp_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
    if (__ballot(rem < 13u || r + 1 >= R.n_reads) == 0ull) {
        const hp_u32x4 a = *reinterpret_cast<const hp_u32x4 *>(g), b = *reinterpret_cast<const hp_u32x4 *>(g + 4), c4 = *reinterpret_cast<const hp_u32x4 *>(g + 8);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        w[8] = c4.x; w[9] = c4.y; w[10] = c4.z; w[11] = c4.w; w[12] = g[12];
    } else {
#pragma unroll
        for (int i = 0; i < 13; i++) w[i] = (uint32_t)i < rem ? g[i] : 0u;
    }
    // the LATTICE class only (positions 8 i): searchCore walks one residue class at a time and leaves it only behind a rejected
    // candidate (libcrispr.cpp:390,295) — 0.76 times per 10 kbp read on BASELINE configs[3] (tools/class_switches.py), so seven
    // of the eight classes this kernel used to cover were never looked at.  The class a walk moves to is covered from there on by
    // the wave that walks (search_core, wave_hints_class)
    uint64_t bits = hint_bits_any<RANGE>(w, 0u, D0, D1);
    // seeds live at j <= searchEnd = L - D0 - 9 (searchCore's loop bound; 58 with the default bounds): the bits behind it — the
    // zero padding matches itself — are cleared, so that a read without a real lattice hint has an all-zero bitmap and the
    // walking wave can drop it without staging it (k_survivor, no_seed)
    const int last = (int)L - D0 - 9 - (int)(tile * 64u);
    bits = last < 0 ? 0ull : (last >= 63 ? bits : (bits & ((2ull << last) - 1ull)));
    hint_bits[t] = bits;
    // the bits as the seed-scan FILTER of a set without a lane-per-read filter (reads of 257 .. 2 048 bases, strides that differ):
    // bit r of the (cleared) hitmask = read r has a hint bit.  With everything behind searchEnd cleared, an all-zero bitmap proves
    // that searchCore's seed loop (libcrispr.cpp:295-348) finds nothing; a superset like the other filters, exception reads as in
    // k_filter_general.  A few per cent of the tiles hold a bit: the atomics are rare
    if (hitmask && bits && (exc_survive || !rd_is_exc(R, r))) atomicOr(reinterpret_cast<unsigned long long *>(hitmask) + (r >> 6), 1ull << (r & 63u));
}

hipError_t launch_hint_positions(const DevReads &R, const DevParams &P, const uint64_t *hint_off, const uint32_t *blk_read, uint64_t n_words,
                                 uint64_t *hint_bits, hipStream_t st, uint64_t w_begin, uint64_t w_end, uint64_t *hitmask)
{
    // the defaults' lattice and window; any shift range the 13-word tile covers (a copy at most 127 bases on)
    if (P.window != 8 || P.skips != 8 || P.lowDR + P.lowSp < 17 || P.highDR + P.highSp > 127 || P.highDR + P.highSp < P.lowDR + P.lowSp) return hipErrorNotSupported;
    if (w_end > n_words) w_end = n_words;
    if ((w_begin & 255u) != 0) return hipErrorInvalidValue;
    if (w_begin >= w_end) return hipSuccess;
    const int D0 = (int)(P.lowDR + P.lowSp), D1 = (int)(P.highDR + P.highSp);
    const dim3 hg((unsigned)((w_end - w_begin + 255) / 256));
    static const int force_hp = getenv("CRASS_HINT_RANGE") ? atoi(getenv("CRASS_HINT_RANGE")) : 0;      // A/B: 1 = the run-time-range form for the hint kernel, 2 = for the light walk, 3 = both
    if (D0 == 49 && D1 == 97 && !(force_hp & 1)) CRASS_LAUNCH(k_hint_positions<false>, hg, dim3(256), 0, st, R, hint_off, blk_read, w_begin, w_end, hint_bits, D0, D1, hitmask, P.exc_survive);
    else CRASS_LAUNCH(k_hint_positions<true>, hg, dim3(256), 0, st, R, hint_off, blk_read, w_begin, w_end, hint_bits, D0, D1, hitmask, P.exc_survive);
    return hipGetLastError();
}

// The seed-scan FILTER of reads of 257 .. 2 048 bases (and of sets whose strides differ) under another window or seed lattice
// (-w, -d): no position hints are kept for those (the walks' hint forms know the default lattice), so a tile's bits are computed,
// cut to the lattice positions j = i * skips <= searchEnd, and only the read's bit in the (cleared) filter mask is set.  A superset
// like every filter here; 11 instructions per word and shift for every position — four times the lattice-class kernel, a fifth of
// k_filter_general, which these sets took until now.
__global__ __launch_bounds__(256) void k_hint_filter_any(DevReads R, DevParams P, const uint64_t *hint_off, const uint32_t *blk_read, uint64_t n_words,
                                                         uint64_t *hitmask, uint64_t *hint_bits)
{
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n_words) return;
    uint64_t r;
    uint32_t tile;
    hint_tile_read(R, hint_off, blk_read, t, n_words, r, tile);
    const uint32_t L = rd_len(R, r);
    const int D0 = (int)(P.lowDR + P.lowSp), D1 = (int)(P.highDR + P.highSp);
    const int last = (int)L - D0 - (int)P.window - 1 - (int)(tile * 64u);        // searchEnd, counted from this tile's first position
    if (last < 0) { hint_bits[t] = 0ull; return; }
    const uint32_t nw = (L + 15) >> 4;
    const uint32_t *g = R.packed + rd_word_off(R, r) + tile * 4u;
    const uint32_t rem = nw - tile * 4u;
    uint32_t w[13];
#pragma unroll
    for (int i = 0; i < 13; i++) w[i] = (uint32_t)i < rem ? g[i] : 0u;
    uint64_t bits = hint_bits_every(w, (int)P.window, D0, D1);
    if (last < 63) bits &= (2ull << last) - 1ull;
    // every position's bit is kept: the survivors' walks step over the positions whose bit is clear, on the lattice and — behind a
    // rejected candidate — off it (DevReads.hint_all)
    hint_bits[t] = bits;
    // the lattice: positions that are multiples of skips
    const uint32_t skips = P.skips;
    if (skips > 1) {
        const uint64_t p0 = (uint64_t)tile * 64u;
        uint32_t b = (uint32_t)((skips - (uint32_t)(p0 % skips)) % skips);
        uint64_t m = 0;
        for (; b < 64u; b += skips) m |= 1ull << b;
        bits &= m;
    }
    if (bits && (P.exc_survive || !rd_is_exc(R, r))) atomicOr(reinterpret_cast<unsigned long long *>(hitmask) + (r >> 6), 1ull << (r & 63u));
}

hipError_t launch_hint_filter_any(const DevReads &R, const DevParams &P, const uint64_t *hint_off, const uint32_t *blk_read, uint64_t n_words,
                                  uint64_t *hitmask, uint64_t *hint_bits, hipStream_t st)
{
    if (P.window < 6 || P.window > 9 || P.skips < 1 || P.lowDR + P.lowSp < 17 || P.highDR + P.highSp > 127 || P.highDR + P.highSp < P.lowDR + P.lowSp) return hipErrorNotSupported;
    if (!n_words) return hipSuccess;
    const uint64_t nb = (n_words + 255) / 256;
    if (nb > 0x7FFFFFFFull) return hipErrorNotSupported;
    CRASS_LAUNCH(k_hint_filter_any, dim3((unsigned)nb), dim3(256), 0, st, R, P, hint_off, blk_read, n_words, hitmask, hint_bits);
    return hipGetLastError();
}

} // namespace crass
