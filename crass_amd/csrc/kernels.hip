// kernels.hip — hand-written HIP kernels for gfx950 (MI355X, CDNA4, wave64): pass 1's search.
//
// The hot path of crass's WorkHorse search (reference citations are relative to the
// crass v1.0.1 tree):
//   pass 1  searchCore / scanRight / extendPreRepeat / qcFoundRepeats / DRLowLexi
//           (src/crass/libcrispr.cpp:170-395,520-1069, ReadHolder.cpp:513-609,
//            PatternMatcher.cpp:26-204)                                     this file
//   pass 2  findSingletons / on_match over an Aho-Corasick automaton
//           (src/crass/libcrispr.cpp:399-518, src/aho-corasick/acism.c:25-106)     pass2.hip
//   ordered compaction, de-duplication and the hand-off blobs of both passes         sinks.hip
//
// Integer/byte work, HBM- and issue-bound: no MFMA.  Reads are 2-bit packed and streamed
// once per pass; wave64 ballot/ffs gives Boyer-Moore's "leftmost occurrence" for free;
// the pass-2 automaton is staged in LDS when it fits.  Compile with -ffp-contract=off:
// qcFoundRepeats' float evaluation order is part of the parity contract.
#include "dev_common.h"
#include "comp_table.h"
#include "lane_find.h"
#include <type_traits>
#include <algorithm>

namespace crass {

static __constant__ CompTable c_comp = make_comp_table();     // reverseComplement table, SeqUtils.cpp:50-59

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

static __device__ __forceinline__ uint32_t lds_code(const uint32_t *w, uint32_t p, uint32_t mask)
{
    uint32_t wi = p >> 4, sh = (p & 15u) * 2u;
    uint64_t v = ((uint64_t)w[wi + 1] << 32) | w[wi];
    return (uint32_t)(v >> sh) & mask;
}

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
// min(halfword, 1) for both halfwords: 0 where the halfword is 0, else 1.  Through the builtin the optimiser turns this into
// two compares, two selects and a permute; the instruction itself is what is wanted.
static __device__ __forceinline__ uint32_t pk_nonzero_u16(uint32_t a)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(0x00010001u));
    return r;
}
typedef uint32_t ff_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
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

// Hint bits of residue class rho for the 64 positions of one hint word: bit (8 i + rho) is set iff the 8-mer at that position
// has a copy 49 .. 97 bases further on (searchCore's seed test, libcrispr.cpp:295-339; a superset: padding and the right clamp
// are ignored).  w[0..12]: the packed words of the chunk and its halo.  R >> 2 rho puts the seeds 8h + rho on the halfword
// lattice, where the test is the short-read filter's: for a shift d, X = R' ^ (R' >> 2d) has a zero halfword h  <=>  the 8-mer
// at 8h (+ rho) re-occurs d further on — {v_alignbit, v_xor, v_pk_min_u16} per word and shift, 49 x 4 x 3 = 588 instructions
// per 64 positions and CLASS (the all-classes form that k_hint_positions used until round 4 took 2 300 for the eight of them).
static __device__ __forceinline__ uint64_t hint_bits_class(const uint32_t (&w)[13], uint32_t rho)
{
    uint32_t v[12];
    const uint32_t rs = 2u * rho;
#pragma unroll
    for (int i = 0; i < 12; i++) v[i] = rs ? ((w[i] >> rs) | (w[i + 1] << (32u - rs))) : w[i];
    uint32_t acc[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (int d = 49; d <= 97; d++) {
        const int q = d >> 4, sh = (d & 15) * 2;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t lo = v[k + q], hi = v[k + q + 1];
            const uint32_t x = (sh ? ((lo >> sh) | (hi << (32 - sh))) : lo) ^ v[k];
            acc[k] = pk_min_u16(acc[k], x);
        }
    }
    // halfword j of word k -> bit 16 k + 8 j + rho: min(halfword, 1) leaves the miss flags in bytes 0 and 2 of each word, one
    // byte permute gathers those of two words into bytes 0..3
    const uint32_t m0 = pk_nonzero_u16(acc[0]), m1 = pk_nonzero_u16(acc[1]), m2 = pk_nonzero_u16(acc[2]), m3 = pk_nonzero_u16(acc[3]);
    const uint32_t lo = __builtin_amdgcn_perm(m1, m0, 0x06040200u) ^ 0x01010101u;
    const uint32_t hi = __builtin_amdgcn_perm(m3, m2, 0x06040200u) ^ 0x01010101u;
    return ((uint64_t)(hi << rho) << 32) | (uint64_t)(lo << rho);
}

// ... for any shift range D0 .. D1 <= 127 (-s / -S / -D with the defaults' lattice and window): the word part of a shift is a
// compile-time loop, the bit offsets inside it a run-time one (k_filter_fast_range has the reasoning); the defaults keep the
// fully unrolled form above
static __device__ __forceinline__ uint64_t hint_bits_class_range(const uint32_t (&w)[13], uint32_t rho, int D0, int D1)
{
    uint32_t v[12];
    const uint32_t rs = 2u * rho;
#pragma unroll
    for (int i = 0; i < 12; i++) v[i] = rs ? ((w[i] >> rs) | (w[i + 1] << (32u - rs))) : w[i];
    uint32_t acc[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (int q = 0; q < 8; q++) {
        if (16 * q + 15 < D0 || 16 * q > D1) continue;
        const int sb_lo = max(0, D0 - 16 * q), sb_hi = min(15, D1 - 16 * q);
        for (int sb = sb_lo; sb <= sb_hi; sb++) {
            const uint32_t sh = (uint32_t)(2 * sb);
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] = pk_min_u16(acc[k], __builtin_amdgcn_alignbit(v[k + q + 1], v[k + q], sh) ^ v[k]);
        }
    }
    const uint32_t m0 = pk_nonzero_u16(acc[0]), m1 = pk_nonzero_u16(acc[1]), m2 = pk_nonzero_u16(acc[2]), m3 = pk_nonzero_u16(acc[3]);
    const uint32_t lo = __builtin_amdgcn_perm(m1, m0, 0x06040200u) ^ 0x01010101u;
    const uint32_t hi = __builtin_amdgcn_perm(m3, m2, 0x06040200u) ^ 0x01010101u;
    return ((uint64_t)(hi << rho) << 32) | (uint64_t)(lo << rho);
}
// (RANGE is a template parameter of the callers: the two forms never share a kernel's register budget)
template <bool RANGE>
static __device__ __forceinline__ uint64_t hint_bits_any(const uint32_t (&w)[13], uint32_t rho, int D0, int D1)
{
    if (RANGE) return hint_bits_class_range(w, rho, D0, D1);
    return hint_bits_class(w, rho);
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

// The every-position form of the scan for one hint word: bit p is set iff the wn-mer at position p has a copy D0 .. D1 further on
// (k_filter_fast_any's test, any window and lattice).  Used by the filter below and by the light walk k_long_light_any.
static __device__ __forceinline__ uint64_t hint_bits_every(const uint32_t (&w)[13], int wn, int D0, int D1)
{
    const int s1 = min(1, wn - 1), s2 = min(2, wn - 1 - s1), s3 = min(4, wn - 1 - s1 - s2), s4 = wn - 1 - s1 - s2 - s3;
    uint32_t nz[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (int q = 0; q < 8; q++) {
        if (16 * q + 15 < D0 || 16 * q > D1) continue;
        const int sb_lo = max(0, D0 - 16 * q), sb_hi = min(15, D1 - 16 * q);
        for (int sb = sb_lo; sb <= sb_hi; sb++) {
            const uint32_t sh = (uint32_t)(2 * sb);
            uint32_t z[5];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const uint32_t x = __builtin_amdgcn_alignbit(w[k + q + 1], w[k + q], sh) ^ w[k];
                z[k] = x | (x >> 1);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) z[k] |= __builtin_amdgcn_alignbit(z[k + 1], z[k], (uint32_t)(2 * s1));
            if (s2 > 0) {
                z[4] |= z[4] >> (2 * s1);
#pragma unroll
                for (int k = 0; k < 4; k++) z[k] |= __builtin_amdgcn_alignbit(z[k + 1], z[k], (uint32_t)(2 * s2));
            }
            if (s3 > 0) {
                z[4] |= z[4] >> (2 * s2);
#pragma unroll
                for (int k = 0; k < 4; k++) z[k] |= __builtin_amdgcn_alignbit(z[k + 1], z[k], (uint32_t)(2 * s3));
            }
            if (s4 > 0) {
                z[4] |= z[4] >> (2 * s3);
#pragma unroll
                for (int k = 0; k < 4; k++) z[k] |= __builtin_amdgcn_alignbit(z[k + 1], z[k], (uint32_t)(2 * s4));
            }
#pragma unroll
            for (int k = 0; k < 4; k++) nz[k] &= z[k];
        }
    }
    // bit 2p of ~nz[k] = a copy exists for position 16 k + p: the even bits of the four words, packed
    auto even16 = [](uint32_t x) {
        x &= 0x55555555u;
        x = (x | (x >> 1)) & 0x33333333u;
        x = (x | (x >> 2)) & 0x0F0F0F0Fu;
        x = (x | (x >> 4)) & 0x00FF00FFu;
        x = (x | (x >> 8)) & 0x0000FFFFu;
        return x;
    };
    const uint32_t lo = even16(~nz[0]) | (even16(~nz[1]) << 16), hi = even16(~nz[2]) | (even16(~nz[3]) << 16);
    return ((uint64_t)hi << 32) | (uint64_t)lo;
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

// ------------------------------------------------------------------------------------
// pass 1, step 2: the survivor kernel — one wave executes the reference's searchCore for
// one read, byte for byte, with wave-parallel inner operations.
// ------------------------------------------------------------------------------------
struct RH {                 // ReadHolder state (ReadHolder.h:440-451), wave-uniform
    uint8_t *seq;           // LDS, L bytes
    int L;
    uint32_t *ss;           // LDS, RH_StartStops
    int nss, cap;
    int replen;             // RH_RepeatLength
    int err;
    uint16_t *rowA, *rowB;  // Levenshtein block-boundary rows (LDS)
    int row_cap;            // entries per row; a longer string makes qc return -3 (the read is redone with full-size rows)
    float *sims;            // LDS scratch for the QC similarities (ss_cap floats)
    const uint32_t *words;  // LDS copy of the 2-bit packed read (+1 zero word), nullptr for exception reads
    uint32_t cmask;         // (1 << 2w) - 1
    int asc_lo, asc_hi;     // packed reads: seq[] holds the ASCII bases of [asc_lo, asc_hi) only (rh_ascii), wave-uniform
    int asc_pad;            // how far beyond the repeats found so far the byte-wise consumers may read
    uint8_t *seq_buf;       // the LDS bytes behind seq; with a window (seq_win != 0) seq = seq_buf - asc_lo, so that seq[pos] still works
    int seq_win;            // bytes of the ASCII window (0: the whole read fits)
    unsigned long long *lprof;  // diagnostics (CRASS_SURV_PROF): this read's phase cycles / counts in LDS, nullptr normally
};
// phases of one read in the wave kernel (CRASS_SURV_PROF=1, tools/longread_phases.py): cycles unless named n_*
enum { PF_TOTAL = 0, PF_STAGE, PF_FIND, PF_SCAN, PF_EXTEND, PF_QC, PF_HINTS, PF_OUT, PF_N_CAND, PF_N_SCANFIND, PF_N_SWITCH, PF_N_QC, PF_LOOP, PF_N_ITER, PF_MAX, PF_READS, PF_SLOTS };
// LDS behind the layout: PF_SLOTS per-read slots, then 4 categories x PF_SLOTS sums of this wave, then 4 x PF_BINS histogram bins
#define PF_BINS 24
#define PF_LDS_WORDS (PF_SLOTS + 4 * PF_SLOTS + 4 * PF_BINS)
#define PROF_T0(h) const unsigned long long _pt0 = (h).lprof ? (unsigned long long)__builtin_readcyclecounter() : 0ull
#define PROF_ADD(h, ph) do { if ((h).lprof) { const unsigned long long _d = (unsigned long long)__builtin_readcyclecounter() - _pt0; if (lane == 0) (h).lprof[ph] += _d; } } while (0)
#define PROF_CNT(h, ph) do { if ((h).lprof && lane == 0) (h).lprof[ph] += 1ull; } while (0)

// leftmost occurrence of seq[pat, pat+plen) in seq[begin, end): PatternMatcher::bmpSearch
// semantics (PatternMatcher.cpp:26-59: -1 for empty text/pattern or pattern longer than text)
static __device__ int wave_find(const uint8_t *seq, int begin, int end, int pat, int plen, int lane)
{
    int tlen = end - begin;
    if (tlen <= 0 || plen <= 0 || plen > tlen) return -1;
    for (int p0 = begin; p0 + plen <= end; p0 += WAVE) {
        int p = p0 + lane;
        bool ok = (p + plen <= end);
        if (ok) {
            for (int k = 0; k < plen; k++) {
                if (seq[p + k] != seq[pat + k]) { ok = false; break; }
            }
        }
        uint64_t m = __ballot(ok);
        if (m) return p0 + (__ffsll((unsigned long long)m) - 1);
    }
    return -1;
}

// same contract on the 2-bit packed copy: a w-mer is one <=18-bit code, so a window compare is
// one LDS word pair + funnel shift per lane instead of w byte compares
static __device__ int wave_find_packed(const uint32_t *words, uint32_t cmask, int begin, int end, int pat, int plen, int lane)
{
    int tlen = end - begin;
    if (tlen <= 0 || plen <= 0 || plen > tlen) return -1;
    const uint32_t sj = uni(lds_code(words, (uint32_t)pat, cmask));
    for (int p0 = begin; p0 + plen <= end; p0 += WAVE) {
        int p = p0 + lane;
        bool ok = (p + plen <= end) && (lds_code(words, (uint32_t)p, cmask) == sj);
        uint64_t m = __ballot(ok);
        if (m) return p0 + (__ffsll((unsigned long long)m) - 1);
    }
    return -1;
}

static __device__ __forceinline__ int rh_find(const RH &h, int begin, int end, int pat, int plen, int lane)
{
    if (h.words) return wave_find_packed(h.words, h.cmask, begin, end, pat, plen, lane);
    return wave_find(h.seq, begin, end, pat, plen, lane);
}

// The byte-wise consumers (extendPreRepeat's column votes, the QC's string comparisons, DRLowLexi) read the bases around the
// repeats found so far, never far from them — a packed read's ASCII copy is expanded for that REGION when they are entered,
// not for the whole read when it is loaded (a 10 kbp read: 10 KB of LDS writes per read against 2.5 KB for the packed words;
// 61 % of random 10 kbp reads meet a candidate, which covers a few hundred bases).  kAscPad bounds how far the consumers
// reach beyond the first repeat's start / the last one's end: one repeat spacing (highDR + highSp, 97 by default) for the
// extensions; RH::asc_pad = that + 32.
static __device__ __forceinline__ void word_to_ascii(uint32_t v, uint32_t o[4]);
static __device__ void rh_ascii(RH &h, int lane)
{
    if (!h.words || h.nss < 2) return;                  // exception reads: the bytes are the read
    int lo = (int)uni(h.ss[0]) - h.asc_pad, hi = (int)uni(h.ss[h.nss - 1]) + h.asc_pad;
    if (lo < 0) lo = 0;
    if (hi > h.L) hi = h.L;
    if (lo >= h.asc_lo && hi <= h.asc_hi) return;       // (wave-uniform)
    const int w0 = lo >> 4, w1 = (hi + 15) >> 4;
    // (only the candidate in hand is ever read: an earlier candidate's region is dropped.)  With a window: the region
    // starts at the buffer's first byte and seq is moved so that seq[pos] addresses it; a region that does not fit sends the
    // read to the launch with the full layout
    if (h.seq_win) {
        if ((w1 - w0) * 16 > h.seq_win) { h.err = 6; return; }
        h.seq = h.seq_buf - w0 * 16;
    }
    for (int wi = w0 + lane; wi < w1; wi += WAVE) {
        uint32_t o[4];
        word_to_ascii(h.words[wi], o);
        uint32_t *dst = reinterpret_cast<uint32_t *>(h.seq + 16 * wi);   // seq region is 16-B aligned and padded
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2]; dst[3] = o[3];
    }
    h.asc_lo = w0 * 16; h.asc_hi = min(w1 * 16, h.L + 16);
    wave_sync();
}

// ReadHolder::startStopsAdd, ReadHolder.cpp:263-297
static __device__ void rh_add(RH &h, uint32_t i, uint32_t j, int lane)
{
    if (h.nss + 2 > h.cap) { h.err = 2; return; }
    if (j >= (uint32_t)h.L) j = (uint32_t)h.L - 1;
    if (lane == 0) { h.ss[h.nss] = i; h.ss[h.nss + 1] = j; }
    h.nss += 2;
    wave_sync();
}

static __device__ void scan_right_masks(RH &h, int pat, uint32_t pattern_length, uint32_t minSpacerLength, uint32_t scanRange,
                                        uint32_t last_repeat_index, uint32_t second_last_repeat_index, int lane);
// scanRight, libcrispr.cpp:170-263
static __device__ void scan_right(RH &h, int pat, uint32_t pattern_length, uint32_t minSpacerLength,
                                  uint32_t scanRange, int lane)
{
    uint32_t last_repeat_index = uni(h.ss[h.nss - 2]);
    uint32_t second_last_repeat_index = uni(h.ss[h.nss - 4]);
    uint32_t repeat_spacing = last_repeat_index - second_last_repeat_index;
    const uint32_t read_length = (uint32_t)h.L;
    bool more_to_search = true;
    while (more_to_search) {
        int candidate_repeat_index = (int)(last_repeat_index + repeat_spacing);
        uint32_t begin_search = (uint32_t)candidate_repeat_index - scanRange;
        uint32_t end_search = (uint32_t)candidate_repeat_index + pattern_length + scanRange;
        uint32_t scanRightMinBegin = last_repeat_index + pattern_length + minSpacerLength;
        if (begin_search < scanRightMinBegin) begin_search = scanRightMinBegin;
        if (begin_search > read_length - 1) return;
        if (end_search > read_length) end_search = read_length;
        if (begin_search >= end_search) return;
        int position = rh_find(h, (int)begin_search, (int)end_search, pat, (int)pattern_length, lane);
        PROF_CNT(h, PF_N_SCANFIND);
        if (position >= 0) {
            uint32_t found = (uint32_t)position;        // wave_find returns absolute positions
            rh_add(h, found, found + pattern_length - 1, lane);
            if (h.err) return;
            second_last_repeat_index = last_repeat_index;
            last_repeat_index = found;
            repeat_spacing = last_repeat_index - second_last_repeat_index;
            if (repeat_spacing < (minSpacerLength + pattern_length)) more_to_search = false;
            else if (h.words && pattern_length <= 9u) {
                // a third repeat: this is an array, not a chance match — the rest of the chain on match masks
                scan_right_masks(h, pat, pattern_length, minSpacerLength, scanRange, last_repeat_index, second_last_repeat_index, lane);
                return;
            }
        } else {
            more_to_search = false;
        }
    }
}

// extendPreRepeat, libcrispr.cpp:520-772.  The per-column A/C/G/T votes run over repeats in lanes.
static __device__ bool extend_pre_repeat_packed(RH &h, int searchWindowLength, int minSpacerLength, int lane);
static __device__ uint32_t extend_pre_repeat(RH &h, int searchWindowLength, int minSpacerLength, int lane)
{
    // packed reads with at most 64 repeats: on the 2-bit words, no ASCII window (defined with the other packed forms below)
    if (h.words && extend_pre_repeat_packed(h, searchWindowLength, minSpacerLength, lane)) return (uint32_t)h.replen;
    rh_ascii(h, lane);
    if (h.err == 6) return 0;                           // (the region does not fit the ASCII window: search_core hands the read over)
    const uint32_t num_repeats = (uint32_t)h.nss / 2;
    h.replen = searchWindowLength;
    int cut_off = (int)(num_repeats - 1);
    if (2 > cut_off) cut_off = 2;
    const uint32_t first_repeat_start_index = h.ss[0];
    const uint32_t last_repeat_start_index = h.ss[h.nss - 2];
    const uint32_t end_index = (uint32_t)h.nss;
    const uint32_t seqlen = (uint32_t)h.L;
    // shortest spacing between consecutive starts (:557-575)
    uint32_t shortest = 0xFFFFFFFFu;
    for (uint32_t i = 2 + 2 * lane; i < end_index; i += 2 * WAVE) {
        uint32_t sp = (uint32_t)((int)h.ss[i] - (int)h.ss[i - 2]);
        shortest = min(shortest, sp);
    }
    for (int off = 32; off > 0; off >>= 1) shortest = min(shortest, (uint32_t)__shfl_xor((int)shortest, off));
    const uint32_t shortest_repeat_spacing = shortest;

    // The reference extends one column per loop iteration (:612-668, :698-740).  Iteration e of the
    // right loop runs with right_extension_length == e, RH_RepeatLength == w+e and, because one more
    // trailing repeat is dropped in EVERY iteration once lastStart+w+e >= L (:614-616),
    // DR_index_end(e) = end_index - 2*max(0, e - (L-lastStart-w) + 1).  Whether column e passes the
    // vote does not depend on the earlier columns, so all columns are evaluated at once — lane = column —
    // and the extension is the number of leading passing columns (capped by max_*_extension_length).
    uint32_t right_extension_length = 0;
    const uint32_t max_right_extension_length = shortest_repeat_spacing - (uint32_t)minSpacerLength;
    {
        const int T = (int)seqlen - (int)last_repeat_start_index - searchWindowLength;     // >= 0
        for (uint32_t e0 = 0; e0 < max_right_extension_length; e0 += WAVE) {
            const uint32_t e = e0 + (uint32_t)lane;
            int drops = (int)e - T + 1;
            if (drops < 0) drops = 0;
            const int dr_index_end = (int)end_index - 2 * drops;
            int cA = 0, cC = 0, cG = 0, cT = 0;
            for (int k = 0; k < dr_index_end; k += 2) {
                const uint32_t pos = h.ss[k] + (uint32_t)searchWindowLength + e;
                if (pos >= seqlen) break;                // starts ascend: every later repeat is off the read too (:624-627)
                const uint8_t ch = h.seq[pos];
                cA += (ch == 'A'); cC += (ch == 'C'); cG += (ch == 'G'); cT += (ch == 'T');
            }
            const bool pass = (e < max_right_extension_length) &&
                              ((cA >= cut_off) || (cC >= cut_off) || (cG >= cut_off) || (cT >= cut_off));
            const uint64_t fails = ~__ballot(pass);
            if (fails) { right_extension_length = e0 + (uint32_t)(__ffsll((unsigned long long)fails) - 1); break; }
            right_extension_length = e0 + WAVE;
        }
    }
    h.replen = searchWindowLength + (int)right_extension_length;

    uint32_t left_extension_length = 0;
    const int test_for_negative = (int)(shortest_repeat_spacing - (uint32_t)h.replen);
    const uint32_t max_left_extension_length = (test_for_negative >= 0) ? (uint32_t)test_for_negative : 0;
    for (uint32_t e0 = 0; e0 < max_left_extension_length; e0 += WAVE) {
        const uint32_t e = e0 + (uint32_t)lane;
        int drops = (int)e - (int)first_repeat_start_index + 1;          // iterations i<=e with firstStart-i <= 0 (:700-704)
        if (drops < 0) drops = 0;
        int cA = 0, cC = 0, cG = 0, cT = 0;
        for (uint32_t k = 2u * (uint32_t)drops; k < end_index; k += 2) {
            const int idx = (int)(h.ss[k] - e - 1);
            uint8_t ch = 0;
            if (idx >= 0 && idx < h.L) ch = h.seq[idx];
            cA += (ch == 'A'); cC += (ch == 'C'); cG += (ch == 'G'); cT += (ch == 'T');
        }
        const bool pass = (e < max_left_extension_length) &&
                          ((cA >= cut_off) || (cC >= cut_off) || (cG >= cut_off) || (cT >= cut_off));
        const uint64_t fails = ~__ballot(pass);
        if (fails) { left_extension_length = e0 + (uint32_t)(__ffsll((unsigned long long)fails) - 1); break; }
        left_extension_length = e0 + WAVE;
    }
    h.replen += (int)left_extension_length;
    wave_sync();
    for (int r = 2 * lane; r + 1 < h.nss; r += 2 * WAVE) {
        uint32_t a = h.ss[r], b = h.ss[r + 1];
        a = (a < left_extension_length) ? 0 : a - left_extension_length;
        b = (b + right_extension_length >= seqlen) ? seqlen - 1 : b + right_extension_length;
        h.ss[r] = a; h.ss[r + 1] = b;
    }
    wave_sync();
    return (uint32_t)h.replen;
}

// isRepeatLowComplexity, libcrispr.cpp:1031-1069
static __device__ bool is_low_complexity(const uint8_t *rep, int n, int lane)
{
    int a = 0, c = 0, g = 0, t = 0, o = 0;
    for (int i0 = 0; i0 < n; i0 += WAVE) {
        int i = i0 + lane;
        bool v = i < n;
        uint8_t ch = v ? rep[i] : 0;
        uint8_t up = ch & 0xDF;          // case-insensitive for letters
        bool isA = v && up == 'A', isC = v && up == 'C', isG = v && up == 'G', isT = v && up == 'T';
        a += __popcll(__ballot(isA)); c += __popcll(__ballot(isC));
        g += __popcll(__ballot(isG)); t += __popcll(__ballot(isT));
        o += __popcll(__ballot(v && !(isA || isC || isG || isT)));
    }
    int cut_off = (int)((double)n * 0.75);
    return (a > cut_off) || (t > cut_off) || (g > cut_off) || (c > cut_off) || (o > cut_off);
}

// value of lane-1 (lane 0 receives 0): one DPP move (v_mov_b32_dpp wave_shr:1), a few cycles,
// instead of a ds_bpermute round trip through the LDS crossbar — the DP below is a dependent
// chain of these, so their latency is the kernel's critical path.
static __device__ __forceinline__ int wave_shr1(int x)
{
    return __builtin_amdgcn_update_dpp(0, x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// PatternMatcher::levenstheinDistance, PatternMatcher.cpp:111-195, as an anti-diagonal wavefront:
// lane = DP row inside a 64-row block, one DP column step per iteration; neighbours arrive by
// lane shuffles, block-boundary rows go through LDS.  The recurrence (including the
// non-standard transposition term for i>2 && j>2) is symmetric in its arguments, so the
// shorter string is put on the rows.
static __device__ int wave_lev(const uint8_t *s, int n, const uint8_t *t, int m,
                               uint16_t *rowA, uint16_t *rowB, int lane)
{
    if (n == 0) return m;
    if (m == 0) return n;
    if (n > m) { const uint8_t *x = s; s = t; t = x; int y = n; n = m; m = y; }
    int res = 0;
    const int nblocks = (n + WAVE - 1) / WAVE;
    for (int b = 0; b < nblocks; b++) {
        const int i = b * WAVE + lane + 1;               // DP row (1-based)
        const bool rowvalid = i <= n;
        const uint8_t s_i = rowvalid ? s[i - 1] : 0;                  // source[i-1]
        const uint8_t s_im = (rowvalid && i >= 2) ? s[i - 2] : 0;     // source[i-2]
        int left = i;                 // M[i][j-1]; M[i][0] = i
        int pa = 0, ppa = 0, pppa = 0;   // `above` values used at the previous three active steps
        const int rows_here = min(WAVE, n - b * WAVE);
        const int steps = m + rows_here - 1;
        const bool more = (b + 1 < nblocks);
        for (int d = 0; d < steps; d++) {
            const int j = d - lane + 1;                  // my column this step
            int up_left = wave_shr1(left);               // lane-1: M[i-1][j]
            int up_pppa = wave_shr1(pppa);               // lane-1: M[i-2][j-2]
            const bool act = rowvalid && j >= 1 && j <= m;
            if (lane == 0) {
                if (b == 0) { up_left = j; up_pppa = 0; }
                else {
                    up_left = (j >= 0 && j <= m) ? (int)rowA[j] : 0;
                    up_pppa = (j >= 2 && j - 2 <= m) ? (int)rowB[j - 2] : 0;
                }
            }
            if (act) {
                const uint8_t t_j = t[j - 1];
                const int above = up_left;
                const int diag = (j == 1) ? (i - 1) : pa;
                const int cost = (s_i == t_j) ? 0 : 1;
                int cell = min(above + 1, min(left + 1, diag + cost));
                if (i > 2 && j > 2) {
                    int trans = up_pppa + 1;
                    if (s_im != t_j) trans++;
                    if (s_i != t[j - 2]) trans++;
                    if (cell > trans) cell = trans;
                }
                pppa = ppa; ppa = pa; pa = above;
                left = cell;
                if (i == n && j == m) res = cell;
                if (more) {
                    if (lane == WAVE - 1) rowA[j] = (uint16_t)cell;       // M[64(b+1)][j]
                    if (lane == WAVE - 2) rowB[j] = (uint16_t)cell;       // M[64(b+1)-1][j]
                }
            }
        }
        if (more) {
            if (lane == WAVE - 1) rowA[0] = (uint16_t)(b * WAVE + WAVE);
            if (lane == WAVE - 2) rowB[0] = (uint16_t)(b * WAVE + WAVE - 1);
            wave_sync();
        }
    }
    // broadcast the result from the lane that owns row n
    const int owner = (n - 1) & (WAVE - 1);
    return __shfl(res, owner);
}

// PatternMatcher::getStringSimilarity, PatternMatcher.cpp:197-204
static __device__ float wave_similarity(const uint8_t *s1, int n, const uint8_t *s2, int m,
                                        uint16_t *rowA, uint16_t *rowB, int lane)
{
    float max_length = (float)(n > m ? n : m);
    if (n < 3 || m < 3) return 0.0f;
    float edit_distance = (float)wave_lev(s1, n, s2, m, rowA, rowB, lane);
    return (float)(1.0 - (double)(edit_distance / max_length));
}

// The same distance, one pair per LANE, bit-parallel (Myers / Hyyro 2003 OSA recurrences on one
// 64-bit column word).  The reference's transposition term only ever lowers a cell when both
// crossed characters match (otherwise M[i-2][j-2]+2 or +3 >= the substitution path), i.e. it is
// the OSA transposition restricted to i>2 && j>2: TR is masked for rows 1,2 (bits 0,1) and for
// the first two text columns.  Needs the shorter string to be <= 64 long and ACGT-only (the
// longer one may hold any byte: it simply matches nothing); returns -1 otherwise and the caller
// falls back to the wavefront version.  Checked against the oracle / compiled reference in
// tests (levenshtein batch + every QC decision of the parity suites).
template <typename WORD>
static __device__ __forceinline__ int lane_lev_bp_core(const uint8_t *s, int n, const uint8_t *t, int m)
{
    // straight-line selects only (masks of 0 / ~0): a per-character if-ladder compiles to a chain of
    // exec-mask branches that dominates the loop
    WORD pA = 0, pC = 0, pG = 0, pT = 0;
    uint32_t bad = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t c = s[i];
        const WORD b = (WORD)1 << i;
        const WORD mA = (WORD)0 - (WORD)(c == 'A'), mC = (WORD)0 - (WORD)(c == 'C');
        const WORD mG = (WORD)0 - (WORD)(c == 'G'), mT = (WORD)0 - (WORD)(c == 'T');
        pA |= b & mA; pC |= b & mC; pG |= b & mG; pT |= b & mT;
        bad |= (uint32_t)((mA | mC | mG | mT) == 0);
    }
    WORD VP = ~(WORD)0, VN = 0, D0 = 0, PMold = 0;
    int dist = n;
    const int topbit = n - 1;
    for (int j = 0; j < m; j++) {
        const uint32_t c = t[j];
        const WORD mA = (WORD)0 - (WORD)(c == 'A'), mC = (WORD)0 - (WORD)(c == 'C');
        const WORD mG = (WORD)0 - (WORD)(c == 'G'), mT = (WORD)0 - (WORD)(c == 'T');
        const WORD PMj = (pA & mA) | (pC & mC) | (pG & mG) | (pT & mT);
        WORD TR = (WORD)((((WORD)~D0) & PMj) << 1) & PMold & ~(WORD)3;
        TR &= (WORD)0 - (WORD)(j >= 2);
        D0 = (WORD)((WORD)((WORD)(PMj & VP) + VP) ^ VP) | PMj | VN;
        D0 |= TR;
        WORD HP = VN | (WORD)~(D0 | VP);
        WORD HN = D0 & VP;
        dist += (int)((HP >> topbit) & 1) - (int)((HN >> topbit) & 1);
        HP = (WORD)(HP << 1) | (WORD)1;
        HN = (WORD)(HN << 1);
        VP = HN | (WORD)~(D0 | HP);
        VN = HP & D0;
        PMold = PMj;
    }
    return bad ? -1 : dist;
}

static __device__ int lane_lev_bp(const uint8_t *s, int n, const uint8_t *t, int m)
{
    if (n == 0) return m;
    if (m == 0) return n;
    if (n > m) { const uint8_t *x = s; s = t; t = x; int y = n; n = m; m = y; }
    if (n > 64) return -1;
    // one 32-bit column word when the shorter string fits: half the VALU work of the 64-bit form
    return (n <= 32) ? lane_lev_bp_core<uint32_t>(s, n, t, m) : lane_lev_bp_core<uint64_t>(s, n, t, m);
}

// getStringSimilarity for one pair per lane; *fallback set when the bit-parallel form does not apply
static __device__ float lane_similarity(const uint8_t *s1, int n, const uint8_t *s2, int m, bool &fallback)
{
    fallback = false;
    float max_length = (float)(n > m ? n : m);
    if (n < 3 || m < 3) return 0.0f;
    int d = lane_lev_bp(s1, n, s2, m);
    if (d < 0) { fallback = true; return 0.0f; }
    float edit_distance = (float)d;
    return (float)(1.0 - (double)(edit_distance / max_length));
}

// std::string::substr(pos, n) length: throws if pos > size
static __device__ __forceinline__ bool substr_len(int L, uint32_t pos, uint32_t n, uint32_t &len)
{
    if (pos > (uint32_t)L) return false;
    uint32_t avail = (uint32_t)L - pos;
    len = n < avail ? n : avail;
    return true;
}

// getStringSimilarity (PatternMatcher.cpp:197-204) of read[s0, s0+n) and read[t0, t0+m), both <= 64 bases, on the packed words:
// ten independent LDS reads, then the bit-parallel distance runs on registers (ln_lev_regs: the lane kernel's form)
template <typename WORD> static __device__ __forceinline__ int ln_lev_regs(uint64_t s_lo, uint64_t s_hi, int n, uint64_t t_lo, uint64_t t_hi, int m, int stop_at);
static __device__ __forceinline__ void wv_load128(const uint32_t *words, int start, uint64_t &lo, uint64_t &hi);
// narrow: every lane of the wave holds a pair whose shorter string has at most 32 bases (or none) — the distance then runs on 32-bit
// words, half the instructions (the caller's ballot: the choice is the wave's, not the lane's)
static __device__ float packed_similarity(const uint32_t *words, uint32_t s0, int n, uint32_t t0, int m, bool narrow = false)
{
    const float max_length = (float)(n > m ? n : m);
    if (n < 3 || m < 3) return 0.0f;
    if (n > m) { const uint32_t x = s0; s0 = t0; t0 = x; const int y = n; n = m; m = y; }
    uint64_t sl, sh, tl, th;
    wv_load128(words, (int)s0, sl, sh); wv_load128(words, (int)t0, tl, th);
    const float edit_distance = narrow ? (float)ln_lev_regs<uint32_t>(sl, sh, n, tl, th, m, -1) : (float)ln_lev_regs<uint64_t>(sl, sh, n, tl, th, m, -1);
    return (float)(1.0 - (double)(edit_distance / max_length));
}

// qcFoundRepeats, libcrispr.cpp:869-1029.  1 pass / 0 fail / -1 reference would throw.
// Internal spacer i (getAllSpacerStrings, ReadHolder.cpp:199-239) = seq[ss[2i+1]+1, ss[2i+2]).
static __device__ int qc_found_repeats(RH &h, int minSpacerLength, int maxSpacerLength, int lane, uint32_t dbg = 0)
{
    rh_ascii(h, lane);
    if (h.err == 6) return -3;
    const int num_repeats = h.nss / 2;
    if (num_repeats < 2) return -1;
    uint32_t rep_len;
    const uint32_t rep_start = uni(h.ss[0]);
    if (!substr_len(h.L, rep_start, uni(h.ss[1]) - rep_start + 1, rep_len)) return -1;
    const uint8_t *repeat = h.seq + rep_start;
    if (is_low_complexity(repeat, (int)rep_len, lane)) return 0;

    bool is_short = (2 > (num_repeats - 1));
    if (!is_short) {
        float ave_spacer_to_spacer_len_difference = 0.0f;
        float ave_repeat_to_spacer_len_difference = 0.0f;
        float ave_spacer_to_spacer_difference = 0.0f;
        float ave_repeat_to_spacer_difference = 0.0f;
        int min_spacer_length = 10000000;
        int max_spacer_length = 0;
        int num_compared = 0;
        const int nsp = num_repeats - 1;
        // The reference walks the spacers once, summing similarities and length differences, and only then tests: spacer lengths,
        // the two similarity averages, the two length-difference averages — every failed test is the same `return false`
        // (:773-867).  The length tests need no edit distance, so they are taken FIRST here: a candidate that fails one of them
        // (the common reason: every other repeat of an array missed, spacers of 100 bases) leaves without a single DP.  One read
        // of BASELINE configs[3] spent 5.3 M cycles — 2.3 ms, the tail of the whole launch — on 54 wavefront DPs of 77 x 77 cells
        // for a candidate whose longest spacer decides it.  (A throw in getAllSpacerStrings comes before any of it: -1.)
        // Terms are fetched by the lanes — lane i: spacer i — and summed lane by lane in the reference's order (float addition
        // does not associate): a term is a v_readlane instead of dependent LDS reads per spacer.
        for (int c0 = 0; c0 < nsp; c0 += WAVE) {
            const int i = c0 + lane;
            const bool vi = i < nsp, vc = i + 1 < nsp;
            uint32_t cur_len = 0, nxt_len = 0;
            bool bad = false;
            if (vi) { const uint32_t cs = h.ss[2 * i + 1] + 1; bad = !substr_len(h.L, cs, h.ss[2 * i + 2] - cs, cur_len); }
            if (vc) { const uint32_t ns = h.ss[2 * i + 3] + 1; bad = bad || !substr_len(h.L, ns, h.ss[2 * i + 4] - ns, nxt_len); }
            if (__ballot(bad)) return -1;
            const float t_ssl = (float)cur_len - (float)nxt_len, t_rsl = (float)rep_len - (float)cur_len;
            int mn = vi ? (int)cur_len : 10000000, mx = vi ? (int)cur_len : 0;
            for (int off = 32; off > 0; off >>= 1) { mn = min(mn, __shfl_xor(mn, off)); mx = max(mx, __shfl_xor(mx, off)); }
            if (mn < min_spacer_length) min_spacer_length = mn;
            if (mx > max_spacer_length) max_spacer_length = mx;
            const int i_end = min(c0 + WAVE, nsp - 1);                 // comparisons i = c0 .. i_end - 1 (i + 1 < nsp)
            for (int ii = c0; ii < i_end; ii++) {
                const int src = ii - c0;
                num_compared++;
                ave_spacer_to_spacer_len_difference += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t_ssl), src));
                ave_repeat_to_spacer_len_difference += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t_rsl), src));
            }
        }
        // num_compared == nsp-1 >= 1 here (the reference's num_compared == 0 branch needs <2 spacers)
        ave_spacer_to_spacer_len_difference /= (float)num_compared;
        ave_spacer_to_spacer_len_difference = fabsf(ave_spacer_to_spacer_len_difference);
        ave_repeat_to_spacer_len_difference /= (float)num_compared;
        ave_repeat_to_spacer_len_difference = fabsf(ave_repeat_to_spacer_len_difference);
        if (min_spacer_length < minSpacerLength) return 0;                 // testSpacerLength :773-800
        if (max_spacer_length > maxSpacerLength) return 0;
        if ((int)ave_spacer_to_spacer_len_difference > 12) return 0;       // int parameter: truncation (:836)
        if ((int)ave_repeat_to_spacer_len_difference > 30) return 0;       // (:853)
        // all 2*(nsp-1) similarities are independent: one pair per lane (bit-parallel DP on the packed words), the float
        // sums below then consume them in the reference's order.  pair 2i = (repeat, spacer_i),
        // pair 2i+1 = (spacer_i, spacer_i+1)   (:921-950)
        // A round of 64 lanes takes pairs of ONE kind — first the (repeat, spacer) pairs, then the (spacer, spacer) pairs: the
        // two kinds side by side in one round were two executions of the distance loop with half the lanes each, and the rounds of
        // the first kind share their shorter string's bound — a repeat of up to 32 bases puts the whole round on 32-bit words.
        // (QC was 46 % of the full kernel's cycles on the array reads of BASELINE configs[3]; NOTES r06.)
        const int per_kind = nsp - 1, rounds_per_kind = (per_kind + WAVE - 1) / WAVE;
        for (int rd = 0; rd < 2 * rounds_per_kind; rd++) {
            const int kind = rd >= rounds_per_kind ? 1 : 0;
            const int i_l = (rd - kind * rounds_per_kind) * WAVE + lane;
            const bool valid = i_l < per_kind;
            const int q = valid ? 2 * i_l + kind : 0;
            const int i = valid ? i_l : 0;
            uint32_t a_start = h.ss[2 * i + 1] + 1, a_len = 0, b_start = h.ss[2 * i + 3] + 1, b_len = 0;
            bool bad = !substr_len(h.L, a_start, h.ss[2 * i + 2] - a_start, a_len);
            bad = bad || !substr_len(h.L, b_start, h.ss[2 * i + 4] - b_start, b_len);
            if (__ballot(valid && bad)) return -1;
            bool fb = false;
            float sim = 0.0f;
            if (valid && dbg != 5) {
                // (packed reads, strings of at most 64 bases — always, with anything like the default bounds: on the 2-bit words)
                const bool pk = h.words && rep_len <= 64u && a_len <= 64u && b_len <= 64u;
                const uint32_t x0 = kind ? a_start : rep_start, xn = kind ? a_len : rep_len, y0 = kind ? b_start : a_start, yn = kind ? b_len : a_len;
                const bool narrow = __ballot(valid && pk && min(xn, yn) > 32u) == 0ull;      // (wave-uniform)
                if (pk) sim = packed_similarity(h.words, x0, (int)xn, y0, (int)yn, narrow);
                else sim = lane_similarity(h.seq + x0, (int)xn, h.seq + y0, (int)yn, fb);
            }
            if (valid) h.sims[q] = sim;
            uint64_t fbmask = __ballot(valid && fb);
            while (fbmask) {                              // rare: > 64-long or non-ACGT shorter string
                const int src = __ffsll((unsigned long long)fbmask) - 1;
                fbmask &= fbmask - 1;
                const int qq = 2 * ((rd - kind * rounds_per_kind) * WAVE + src) + kind, ii = qq >> 1;      // (lane src's pair)
                uint32_t as = h.ss[2 * ii + 1] + 1, al = 0, bs = h.ss[2 * ii + 3] + 1, bl = 0;
                (void)substr_len(h.L, as, h.ss[2 * ii + 2] - as, al);
                (void)substr_len(h.L, bs, h.ss[2 * ii + 4] - bs, bl);
                if ((int)std::max(std::max(al, bl), rep_len) + 8 > h.row_cap) return -3;
                float sw = (qq & 1) ? wave_similarity(h.seq + as, (int)al, h.seq + bs, (int)bl, h.rowA, h.rowB, lane)
                                    : wave_similarity(repeat, (int)rep_len, h.seq + as, (int)al, h.rowA, h.rowB, lane);
                if (lane == 0) h.sims[qq] = sw;
            }
        }
        wave_sync();
        for (int c0 = 0; c0 + 1 < nsp; c0 += WAVE) {
            const int i = c0 + lane;
            const bool vc = i + 1 < nsp;
            const float t_rs = vc ? h.sims[2 * i] : 0.0f, t_ss = vc ? h.sims[2 * i + 1] : 0.0f;
            const int i_end = min(c0 + WAVE, nsp - 1);
            for (int ii = c0; ii < i_end; ii++) {
                const int src = ii - c0;
                ave_repeat_to_spacer_difference += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t_rs), src));
                float ss_diff = 0;
                ss_diff += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t_ss), src));
                ave_spacer_to_spacer_difference += ss_diff;
            }
        }
        wave_sync();
        ave_spacer_to_spacer_difference /= (float)num_compared;
        ave_repeat_to_spacer_difference /= (float)num_compared;
        if ((double)ave_spacer_to_spacer_difference > 0.82) return 0;      // :802-834
        if ((double)ave_repeat_to_spacer_difference > 0.82) return 0;
    }
    if (is_short) {
        // spacerStringAt(0), ReadHolder.cpp:102-147 — one base short
        uint32_t s = h.ss[1] + 1;
        uint32_t e = h.ss[2] - 1;
        uint32_t sp_len;
        if (!substr_len(h.L, s, e - s, sp_len)) return -1;
        if ((int)sp_len < minSpacerLength) return 0;
        if ((int)sp_len > maxSpacerLength) return 0;
        bool fb = false;
        const bool pk = h.words && rep_len <= 64u && sp_len <= 64u;
        float similarity = (dbg == 5) ? 0.0f : (pk ? packed_similarity(h.words, rep_start, (int)rep_len, s, (int)sp_len)
                                                   : lane_similarity(repeat, (int)rep_len, h.seq + s, (int)sp_len, fb));     // same pair in every lane
        if (fb && (int)std::max(sp_len, rep_len) + 8 > h.row_cap) return -3;
        if (fb) similarity = wave_similarity(repeat, (int)rep_len, h.seq + s, (int)sp_len, h.rowA, h.rowB, lane);
        if ((double)similarity > 0.82) return 0;
        int dlen = (int)sp_len - (int)rep_len;
        if (dlen < 0) dlen = -dlen;
        if (dlen > 30) return 0;
    }
    return 1;
}

// ------------------------------------------------------------------------------------
// Packed reads in the wave kernel: scanRight, extendPreRepeat and the QC's edit distances on the 2-bit words in LDS — no
// ASCII window, no per-base LDS round trips.  One long read costs the wave (phase counters, CRASS_SURV_PROF, 1 M x 10 kbp):
// an array read 234 k cycles, of which the QC 128 k (two dependent LDS byte reads per DP column and lane), the scanRight chain
// 52 k (38 finds x {two LDS round trips + a ballot + two fenced list appends}), the extension 31 k (a lane per COLUMN walks the
// 36 repeats, two dependent LDS reads each); a read without an array 27 k, 4.3 k of them a two-repeat extension.  The forms
// below keep the reference's decisions and arithmetic (libcrispr.cpp:170-263, 520-772, 869-1029) and change what a lane holds.
// ------------------------------------------------------------------------------------
template <typename WORD> static __device__ __forceinline__ int ln_lev_regs(uint64_t s_lo, uint64_t s_hi, int n, uint64_t t_lo, uint64_t t_hi, int m, int stop_at);
static __device__ __forceinline__ int ln_run_up(uint64_t x0, uint64_t x1, int n);
static __device__ __forceinline__ int ln_run_down(uint64_t x0, uint64_t x1, int n);

// bases [start, start + 64) of the read as two 64-bit words (base `start` in bits 0-1); start >= 0.  Words past the read are
// whatever the LDS holds there: every consumer masks by its own length.
static __device__ __forceinline__ void wv_load128(const uint32_t *words, int start, uint64_t &lo, uint64_t &hi)
{
    const int wi = start >> 4;
    const uint32_t sh = (uint32_t)(start & 15) * 2u;
    const uint32_t a0 = words[wi], a1 = words[wi + 1], a2 = words[wi + 2], a3 = words[wi + 3], a4 = words[wi + 4];
    const uint32_t y0 = __builtin_amdgcn_alignbit(a1, a0, sh), y1 = __builtin_amdgcn_alignbit(a2, a1, sh);
    const uint32_t y2 = __builtin_amdgcn_alignbit(a3, a2, sh), y3 = __builtin_amdgcn_alignbit(a4, a3, sh);
    lo = (uint64_t)y0 | ((uint64_t)y1 << 32); hi = (uint64_t)y2 | ((uint64_t)y3 << 32);
}
// ... the 64 bases that END before `end` (bases [end - 64, end)), base end - 64 in bits 0-1; positions before the read's
// first base read as 0 (the callers never count them)
static __device__ __forceinline__ void wv_load128_before(const uint32_t *words, int end, uint64_t &lo, uint64_t &hi)
{
    const int start = end - 64;
    if (start >= 0) { wv_load128(words, start, lo, hi); return; }
    uint64_t l, h2;
    wv_load128(words, 0, l, h2);
    const int s = -2 * start;                           // bit positions to move up: 2 .. 128
    if (s >= 128) { lo = 0; hi = 0; }
    else if (s >= 64) { lo = 0; hi = s == 64 ? l : (l << (s - 64)); }
    else { hi = (h2 << s) | (l >> (64 - s)); lo = l << s; }
}
static __device__ __forceinline__ uint32_t wv_base(uint64_t lo, uint64_t hi, int i)     // base i of a 128-bit piece, 0 <= i < 64
{
    return (uint32_t)((i < 32 ? lo >> (2 * i) : hi >> (2 * (i - 32))) & 3ull);
}

// extendPreRepeat (libcrispr.cpp:520-772) on the packed words.  Two repeats: the closed form of the lane kernel (ln_extend2:
// cut_off = 2, a column passes iff both copies agree, so the extensions are runs of equal bases).  3 .. 64 repeats: a LANE PER
// REPEAT holds the 64 bases right of its window (then left of it) in registers and a column's vote is four ballots — the
// columns are taken in the reference's order and stop at the first that fails.  Returns false when it does not apply (more than
// 64 repeats: the column-parallel form below takes those).
static __device__ bool extend_pre_repeat_packed(RH &h, int searchWindowLength, int minSpacerLength, int lane)
{
    const int nrep = h.nss / 2;
    if (nrep < 2 || nrep > WAVE) return false;
    const int L = h.L, w = searchWindowLength;
    const uint32_t *words = h.words;
    uint32_t right = 0, left = 0;
    if (nrep == 2) {
        const int j = (int)uni(h.ss[0]), p = (int)uni(h.ss[2]);
        const int spacing = p - j;
        int max_right = spacing - minSpacerLength;                  // (unsigned in the reference; spacing >= minSpacer + w here)
        if (max_right > L - (p + w)) max_right = L - (p + w);       // the second copy's column must lie inside the read
        int rr = 0;
        while (rr < max_right) {
            uint64_t a0, a1, b0, b1;
            wv_load128(words, j + w + rr, a0, a1); wv_load128(words, p + w + rr, b0, b1);
            const int n = max_right - rr < 64 ? max_right - rr : 64;
            const int r = uni(ln_run_up(a0 ^ b0, a1 ^ b1, n));
            rr += r;
            if (r < n) break;
        }
        const int len_r = w + rr;
        int max_left = spacing - len_r;
        if (max_left < 0) max_left = 0;
        if (max_left > j) max_left = j;                             // the first copy's column must lie inside the read
        int ll = 0;
        while (ll < max_left) {
            const int n = max_left - ll < 64 ? max_left - ll : 64;
            uint64_t a0, a1, b0, b1;
            wv_load128(words, j - ll - n, a0, a1); wv_load128(words, p - ll - n, b0, b1);
            const int r = uni(ln_run_down(a0 ^ b0, a1 ^ b1, n));
            ll += r;
            if (r < n) break;
        }
        right = (uint32_t)rr; left = (uint32_t)ll;
    } else {
        const int cut_off = nrep - 1;                               // (max(2, nrep - 1) with nrep >= 3)
        const uint32_t end_index = (uint32_t)h.nss;
        const uint32_t first_start = uni(h.ss[0]), last_start = uni(h.ss[h.nss - 2]);
        const uint32_t seqlen = (uint32_t)L;
        const bool mine = lane < nrep;
        const uint32_t my_start = mine ? h.ss[2 * lane] : 0u;
        uint32_t shortest = 0xFFFFFFFFu;
        if (mine && lane > 0) shortest = (uint32_t)((int)my_start - (int)h.ss[2 * lane - 2]);
        for (int off = 32; off > 0; off >>= 1) shortest = min(shortest, (uint32_t)__shfl_xor((int)shortest, off));
        shortest = uni(shortest);
        const uint32_t max_right = shortest - (uint32_t)minSpacerLength;
        const int T = (int)seqlen - (int)last_start - w;           // >= 0
        bool stop = false;
        for (uint32_t e0 = 0; e0 < max_right && !stop; e0 += 64u) {
            uint64_t lo = 0, hi = 0;
            if (mine) wv_load128(words, (int)(my_start + (uint32_t)w + e0), lo, hi);
            const uint32_t e1 = min(e0 + 64u, max_right);
            for (uint32_t e = e0; e < e1; e++) {
                int drops = (int)e - T + 1;
                if (drops < 0) drops = 0;
                const int n_part = nrep - drops;                    // DR_index_end / 2 of this iteration (:614-616)
                const uint32_t pos = my_start + (uint32_t)w + e;
                const bool valid = mine && lane < n_part && pos < seqlen;     // (starts ascend: behind the first repeat off the read nobody votes, :624-627)
                const uint32_t b = wv_base(lo, hi, (int)(e - e0));
                const int cA = __popcll(__ballot(valid && b == 0u)), cC = __popcll(__ballot(valid && b == 1u));
                const int cG = __popcll(__ballot(valid && b == 2u)), cT = __popcll(__ballot(valid && b == 3u));
                if ((cA >= cut_off) || (cC >= cut_off) || (cG >= cut_off) || (cT >= cut_off)) right++;
                else { stop = true; break; }
            }
        }
        const int replen_r = w + (int)right;
        const int test_for_negative = (int)(shortest - (uint32_t)replen_r);
        const uint32_t max_left = (test_for_negative >= 0) ? (uint32_t)test_for_negative : 0u;
        stop = false;
        for (uint32_t e0 = 0; e0 < max_left && !stop; e0 += 64u) {
            uint64_t lo = 0, hi = 0;
            if (mine) wv_load128_before(words, (int)my_start - (int)e0, lo, hi);      // bases [my_start - e0 - 64, my_start - e0)
            const uint32_t e1 = min(e0 + 64u, max_left);
            for (uint32_t e = e0; e < e1; e++) {
                int drops = (int)e - (int)first_start + 1;          // iterations i <= e with firstStart - i <= 0 (:700-704)
                if (drops < 0) drops = 0;
                const int idx = (int)my_start - (int)e - 1;
                const bool valid = mine && lane >= drops && idx >= 0 && idx < L;
                const uint32_t b = wv_base(lo, hi, 63 - (int)(e - e0));
                const int cA = __popcll(__ballot(valid && b == 0u)), cC = __popcll(__ballot(valid && b == 1u));
                const int cG = __popcll(__ballot(valid && b == 2u)), cT = __popcll(__ballot(valid && b == 3u));
                if ((cA >= cut_off) || (cC >= cut_off) || (cG >= cut_off) || (cT >= cut_off)) left++;
                else { stop = true; break; }
            }
        }
        (void)end_index;
    }
    h.replen = w + (int)right + (int)left;
    wave_sync();
    for (int r = 2 * lane; r + 1 < h.nss; r += 2 * WAVE) {
        uint32_t a = h.ss[r], b = h.ss[r + 1];
        a = (a < left) ? 0 : a - left;
        b = (b + right >= (uint32_t)L) ? (uint32_t)L - 1 : b + right;
        h.ss[r] = a; h.ss[r + 1] = b;
    }
    wave_sync();
    return true;
}

// scanRight's chain (libcrispr.cpp:170-263) once a third repeat exists: instead of one wave-wide find per link — each a pair of
// LDS round trips, a ballot and a fenced append — the wave marks every position of the next 4 096 bases that holds the window's
// w-mer (lane l: the 64 positions from base + 64 l, one bit each) and then follows the chain on those masks: a link is two
// lane reads and a find-first-set.  Entered with last / second-last repeat starts; appends to the start/stop list like rh_add.
static __device__ void scan_right_masks(RH &h, int pat, uint32_t pattern_length, uint32_t minSpacerLength, uint32_t scanRange,
                                        uint32_t last_repeat_index, uint32_t second_last_repeat_index, int lane)
{
    const uint32_t read_length = (uint32_t)h.L;
    const uint32_t sj = uni(lds_code(h.words, (uint32_t)pat, h.cmask));
    last_repeat_index = uni(last_repeat_index); second_last_repeat_index = uni(second_last_repeat_index);
    uint32_t repeat_spacing = last_repeat_index - second_last_repeat_index;
    uint32_t base = 0xFFFFFFFFu;                        // first position the masks cover (a multiple of 64); none yet
    uint64_t mask = 0;
    int nss = h.nss;
    for (;;) {
        // (the chain's state is the same in every lane; said once per link it stays on the scalar unit)
        last_repeat_index = uni(last_repeat_index); repeat_spacing = uni(repeat_spacing); base = uni(base); nss = uni(nss);
        const int candidate_repeat_index = (int)(last_repeat_index + repeat_spacing);
        uint32_t begin_search = (uint32_t)candidate_repeat_index - scanRange;
        uint32_t end_search = (uint32_t)candidate_repeat_index + pattern_length + scanRange;
        const uint32_t scanRightMinBegin = last_repeat_index + pattern_length + minSpacerLength;
        if (begin_search < scanRightMinBegin) begin_search = scanRightMinBegin;
        if (begin_search > read_length - 1) break;
        if (end_search > read_length) end_search = read_length;
        if (begin_search >= end_search) break;
        if (end_search - begin_search < pattern_length) break;          // bmpSearch: pattern longer than the text => -1 => the chain ends
        const uint32_t last_p = end_search - pattern_length;            // the window's last start
        if (base == 0xFFFFFFFFu || begin_search < base || last_p >= base + 4096u) {
            base = begin_search & ~63u;
            const uint32_t p0 = base + 64u * (uint32_t)lane;
            uint64_t m = 0;
            if (p0 + pattern_length <= read_length) {
                const uint32_t wi = p0 >> 4;
                uint32_t a[5];
#pragma unroll
                for (int i = 0; i < 5; i++) a[i] = h.words[wi + i];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint64_t v = ((uint64_t)a[q + 1] << 32) | a[q];
                    uint32_t bits = 0;
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        // (w <= 9: a window of 18 bits starting at bit 2 i <= 30 ends inside the 64-bit piece)
                        const uint32_t c = (uint32_t)(v >> (2 * i)) & h.cmask;
                        bits |= (uint32_t)(c == sj) << i;
                    }
                    m |= (uint64_t)bits << (16 * q);
                }
                // positions whose window would pass the read's end hold no match
                const uint32_t n_ok = read_length - pattern_length - p0 + 1u;      // >= 1 here
                if (n_ok < 64u) m &= (1ull << n_ok) - 1ull;
            }
            mask = m;
        }
        const uint32_t lo_i = begin_search - base, hi_i = last_p - base;      // inclusive bit range, < 4096, at most 57 wide
        const int k0 = (int)(lo_i >> 6), k1 = (int)(hi_i >> 6);
        const uint32_t mlo0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mask, k0), mhi0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mask >> 32), k0);
        uint64_t m0 = (((uint64_t)mhi0 << 32) | mlo0) & (~0ull << (lo_i & 63u));
        if (k1 == k0) m0 &= (hi_i & 63u) == 63u ? ~0ull : ((2ull << (hi_i & 63u)) - 1ull);
        int position = -1;
        if (m0) position = (int)(base + 64u * (uint32_t)k0) + (__ffsll((unsigned long long)m0) - 1);
        else if (k1 > k0) {
            const uint32_t mlo1 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mask, k1), mhi1 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mask >> 32), k1);
            const uint64_t m1 = (((uint64_t)mhi1 << 32) | mlo1) & ((hi_i & 63u) == 63u ? ~0ull : ((2ull << (hi_i & 63u)) - 1ull));
            if (m1) position = (int)(base + 64u * (uint32_t)k1) + (__ffsll((unsigned long long)m1) - 1);
        }
        if (position < 0) break;
        const uint32_t found = (uint32_t)position;
        if (nss + 2 > h.cap) { h.err = 2; break; }                      // (rh_add)
        uint32_t stop = found + pattern_length - 1;
        if (stop >= read_length) stop = read_length - 1;
        if (lane == 0) { h.ss[nss] = found; h.ss[nss + 1] = stop; }
        nss += 2;
        second_last_repeat_index = last_repeat_index;
        last_repeat_index = found;
        repeat_spacing = last_repeat_index - second_last_repeat_index;
        if (repeat_spacing < (minSpacerLength + pattern_length)) break;
    }
    h.nss = nss;
    wave_sync();
}

// searchCore, libcrispr.cpp:265-395.  1 found / 0 not / <0 error
// Hint bits of residue class rho for the read in LDS (h.words), hint words [first_word, end): lanes over hint words, OR-ed into
// the read's hint bitmap (classes occupy disjoint bit positions).  Called by search_core when the walk moves to a class whose
// bits are not there yet from that point on.
template <bool RANGE>
static __device__ __attribute__((noinline)) void wave_hints_class(const RH &h, uint32_t rho, uint32_t first_word, uint64_t *l_hint, int lane, int D0, int D1)
{
    const uint32_t nw = ((uint32_t)h.L + 15u) >> 4, nh = ((uint32_t)h.L + 63u) >> 6;
    for (uint32_t base = first_word; base < nh; base += WAVE) {
        const uint32_t t = base + (uint32_t)lane;
        if (t < nh) {
            uint32_t w[13];
#pragma unroll
            for (int i = 0; i < 13; i++) { const uint32_t wi = 4u * t + (uint32_t)i; w[i] = wi < nw ? h.words[wi] : 0u; }
            l_hint[t] |= hint_bits_any<RANGE>(w, rho, D0, D1);
        }
    }
    wave_sync();
}

// pos_hint (long reads, LDS): the read's per-position hint bits — the lattice class from k_hint_positions; cls_from[rho] (LDS):
// first position from which class rho's bits are in pos_hint (0xFFFFFFFF: not at all)
static __device__ int search_core(RH &h, const DevParams &o, uint32_t seed_hint, int lane, uint64_t *pos_hint = nullptr, uint32_t *cls_from = nullptr,
                                  uint32_t j_start = 0)      // j_start: the light walk has done the iterations before it (all no-ops or rejected candidates)
{
    const uint32_t seq_length = (uint32_t)h.L;
    const uint32_t skips = o.skips;
    int searchEnd = (int)(seq_length - o.lowDR - o.lowSp - o.window - 1);
    if (searchEnd < 0) return 0;
    h.nss = 0;
    // seed_hint (from the bit-parallel filter): bit i clear => lattice seed j = i*skips provably has
    // no hit, so its iteration is a no-op in the reference (no start/stops, numRepeats 0) and can be
    // skipped.  Only valid while j is still on the lattice, i.e. before the first `j = back()-1`.
    bool on_lattice = j_start == 0;
    uint32_t lattice_i = 0;
    for (uint32_t j = j_start; j <= (uint32_t)searchEnd; j = j + skips) {
        j = uni(j);
        PROF_CNT(h, PF_N_ITER);
        if (pos_hint) {
            PROF_T0(h);
            // per-position hints: a clear bit makes this iteration a no-op in the reference, on or off the lattice.  The walk
            // stays on one residue class mod 8 until a rejected candidate moves it (j = back() - 1 below); the bits of the class
            // it moves to are computed here, from this position to the end of the read (the walk only moves forward)
            if (cls_from && j < uni(cls_from[j & 7u])) {     // wave-uniform; never true on the lattice class
                const uint32_t first_word = j >> 6;
                { const unsigned long long _ph0 = h.lprof ? (unsigned long long)__builtin_readcyclecounter() : 0ull;
                { const int D0 = (int)(o.lowDR + o.lowSp), D1 = (int)(o.highDR + o.highSp);
                  if (D0 == 49 && D1 == 97) wave_hints_class<false>(h, j & 7u, first_word, pos_hint, lane, D0, D1);
                  else wave_hints_class<true>(h, j & 7u, first_word, pos_hint, lane, D0, D1); }
                if (h.lprof && lane == 0) { h.lprof[PF_HINTS] += (unsigned long long)__builtin_readcyclecounter() - _ph0; h.lprof[PF_N_SWITCH] += 1ull; } }
                if (lane == 0) cls_from[j & 7u] = first_word << 6;
                wave_sync();
            }
            // With skips == 8 the next candidate in the same 64-bit word is one ffs away.
            const uint64_t wbits = uni64(pos_hint[j >> 6]) >> (j & 63u);
            if (!(wbits & 1ull)) {
                if (skips == 8) {
                    const uint64_t m = wbits & 0x0101010101010101ull;        // positions j, j+8, ... inside this word
                    if (m) j += (uint32_t)(__ffsll((unsigned long long)m) - 1) - 8;    // the loop adds 8: lands on it
                    else {
                        // nothing left in this word: the lanes look at the next 64 hint words at once (a random 10 kbp read
                        // has one or two words with a candidate out of 157; walking them one dependent load at a time was
                        // most of this kernel's time on long reads).  64 is a multiple of the stride, so the candidates of
                        // every later word sit at bit offsets (j mod 8) + 8k.
                        const uint64_t resmask = 0x0101010101010101ull << (j & 7u);
                        const uint32_t n_words = ((uint32_t)searchEnd >> 6) + 1u;
                        uint32_t next_j = 0xFFFFFFFFu;
                        for (uint32_t w0 = (j >> 6) + 1u; w0 < n_words; w0 += 64u) {
                            const uint32_t w = w0 + (uint32_t)lane;
                            const uint64_t v = w < n_words ? (pos_hint[w] & resmask) : 0ull;
                            const uint64_t any = __ballot(v != 0ull);
                            if (any) {
                                const uint32_t fw = w0 + (uint32_t)(__ffsll((unsigned long long)any) - 1);
                                const uint64_t fv = uni64(pos_hint[fw]) & resmask;      // (wave-uniform reload)
                                next_j = fw * 64u + (uint32_t)(__ffsll((unsigned long long)fv) - 1);
                                break;
                            }
                        }
                        if (next_j == 0xFFFFFFFFu) { PROF_ADD(h, PF_LOOP); break; }          // no candidate up to searchEnd: the loop ends
                        j = next_j - 8u;                                            // the loop adds 8: lands on it
                    }
                }
                PROF_ADD(h, PF_LOOP);
                continue;
            }
            PROF_ADD(h, PF_LOOP);
        } else if (on_lattice) {
            const uint32_t li = lattice_i++;
            if (li < 32 && !((seed_hint >> li) & 1u)) continue;
        }
        uint32_t beginSearch = j + o.lowDR + o.lowSp;
        uint32_t endSearch = j + o.highDR + o.highSp + o.window;
        if (endSearch >= seq_length) endSearch = seq_length - 1;
        if (endSearch < beginSearch) endSearch = beginSearch;
        if (beginSearch > seq_length) return -1;                       // substr would throw
        int pos;
        { PROF_T0(h);
        pos = rh_find(h, (int)beginSearch, (int)endSearch, (int)j, (int)o.window, lane);
        PROF_ADD(h, PF_FIND); PROF_CNT(h, PF_N_CAND); }
        if (o.debug_stop == 2) pos = -1;
        if (pos >= 0) {
            PROF_T0(h);
            rh_add(h, j, j + o.window - 1, lane);
            rh_add(h, (uint32_t)pos, (uint32_t)pos + o.window - 1, lane);
            if (h.err) return -2;
            scan_right(h, (int)j, o.window, o.lowSp, 24, lane);
            if (h.err) return -2;
            PROF_ADD(h, PF_SCAN);
        }
        if ((uint32_t)(h.nss / 2) >= o.minRepeats) {
            uint32_t actual_repeat_length;
            { PROF_T0(h);
            actual_repeat_length = extend_pre_repeat(h, (int)o.window, (int)o.lowSp, lane);
            PROF_ADD(h, PF_EXTEND); }
            if (h.err == 6) return -3;
            if (o.debug_stop != 3 && (actual_repeat_length >= o.lowDR) && (actual_repeat_length <= o.highDR)) {
                PROF_T0(h);
                int qc = qc_found_repeats(h, (int)o.lowSp, (int)o.highSp, lane, o.debug_stop);
                PROF_ADD(h, PF_QC); PROF_CNT(h, PF_N_QC);
                if (qc == -3) return -3;
                if (qc < 0) return -1;
                if (qc) return 1;
            }
            j = uni(h.ss[h.nss - 1]) - 1;
            on_lattice = false;
        }
        h.nss = 0;
        wave_sync();
    }
    return 0;
}

// ReadHolder::DRLowLexi + reverseStartStops (ReadHolder.cpp:513-591, 321-380).  Writes the
// low-lexi DR to dr_out (global), mirrors ss in LDS if the read is flipped; returns dr length
// (<0 error) and the RH_WasLowLexi flag.
static __device__ int dr_low_lexi(RH &h, char *dr_out, int dr_stride, int &was_low_lexi, int lane)
{
    rh_ascii(h, lane);
    const int num_repeats = h.nss / 2;
    int pick;
    if (num_repeats == 1) pick = 0;
    else if (num_repeats == 2) {
        if (h.ss[0] == 0) pick = 2;
        else if (h.ss[h.nss - 1] == (uint32_t)h.L) pick = 0;          // dead branch, kept (:541)
        else {
            int lenA = (int)(h.ss[1] - h.ss[0]);
            int lenB = (int)(h.ss[3] - h.ss[2]);
            pick = (lenA > lenB) ? 0 : 2;
        }
    } else pick = 2;
    uint32_t dlen;
    const uint32_t dr_start = uni(h.ss[pick]);
    if (!substr_len(h.L, dr_start, uni(h.ss[pick + 1]) - dr_start + 1, dlen)) return -1;
    const uint8_t *dr = h.seq + dr_start;
    // tmp_dr < rev_comp ?  (std::string operator<, unsigned bytes; equal => not less => flip)
    int less = 0;
    for (int i0 = 0; i0 < (int)dlen; i0 += WAVE) {
        int i = i0 + lane;
        uint8_t a = 0, b = 0;
        if (i < (int)dlen) { a = dr[i]; b = c_comp.v[dr[dlen - 1 - i] & 127]; }
        uint64_t m = __ballot(a != b);
        if (m) {
            int f = __ffsll((unsigned long long)m) - 1;
            int av = __shfl((int)a, f), bv = __shfl((int)b, f);
            less = av < bv;
            break;
        }
    }
    if (less) {
        for (int i = lane; i < dr_stride; i += WAVE) dr_out[i] = (i < (int)dlen) ? (char)dr[i] : (char)0;   // zero padding: slots are bit-reproducible
        was_low_lexi = 1;
    } else {
        for (int i = lane; i < dr_stride; i += WAVE) dr_out[i] = (i < (int)dlen) ? (char)c_comp.v[dr[dlen - 1 - i] & 127] : (char)0;
        // reverseStartStops: new[k] = L-1 - ss[nss-1-k]
        wave_sync();
        for (int k0 = 0; k0 < h.nss; k0 += WAVE) {       // read everything of a chunk pair-wise before writing
            int k = k0 + lane;
            int mirror = h.nss - 1 - k;
            // swap in place: handle k < mirror pairs only
            if (k < h.nss && k < mirror) {
                uint32_t a = h.ss[k], b = h.ss[mirror];
                h.ss[k] = (uint32_t)h.L - 1 - b;
                h.ss[mirror] = (uint32_t)h.L - 1 - a;
            }
        }
        wave_sync();
        was_low_lexi = 0;
    }
    return (int)dlen;
}

// 16 bases of a packed word as ASCII, four letters per output word: the byte of four codes is placed in both 16-bit
// halves (v_perm), the upper half shifted by 4 (v_pk_lshrrev_b16), `u | u << 6` puts each half's second code into its
// upper byte, and the 2-bit codes select from the letters with a second v_perm: 5 instructions per 4 bases instead of ~20
static __device__ __forceinline__ void word_to_ascii(uint32_t v, uint32_t o[4])
{
    const uint32_t letters = ('A') | ('C' << 8) | ('G' << 16) | ('T' << 24);
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t t = __builtin_amdgcn_perm(0u, v, 0x0C000C00u | ((uint32_t)q << 16) | (uint32_t)q);   // [b, 0, b, 0], b = byte q of v
        us2 u2 = __builtin_bit_cast(us2, t);
        u2.y = (unsigned short)(u2.y >> 4);
        const uint32_t u = __builtin_bit_cast(uint32_t, u2);
        const uint32_t sel = (u | (u << 6)) & 0x03030303u;
        o[q] = __builtin_amdgcn_perm(0u, letters, sel);
    }
}

// words of the read a wave works on NEXT, requested while it searches the current one (wave-per-read kernel, long reads:
// a 10 kbp read is ten dependent rounds of loads per lane otherwise — 5.0 of the kernel's 12.3 ms at 1 M x 10 kbp)
#define SV_PREFETCH_WORDS 12                      // per lane: reads up to 12 * 64 * 16 = 12 288 bases are covered completely
#define SV_PREFETCH_HINTS (SV_PREFETCH_WORDS / 4)  // 64-bit hint words per lane for the same reads (one bit per position)
// (the words travel 16 bytes per lane and load: a read is word-aligned, not 16-byte aligned, and the hardware takes a
// dword-aligned global_load_dwordx4 — a quarter of the load and LDS-store instructions of the one-word form)
typedef uint32_t sv_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
#define SV_PREFETCH_VEC (SV_PREFETCH_WORDS / 4)
struct ReadPrefetch {
    uint4 v[SV_PREFETCH_VEC];                     // lane's 16-byte groups lane, lane + 64, ...: words 4 g .. 4 g + 3
    uint64_t hw[SV_PREFETCH_HINTS];
    uint64_t r;                                   // the read these words belong to (~0: none)
};
// group gi (words 4 gi .. 4 gi + 3) of a read of nw words at g; words past the read are 0 and never touched in memory
static __device__ __forceinline__ uint4 sv_load_group(const uint32_t *g, int gi, int nw)
{
    uint4 v; v.x = v.y = v.z = v.w = 0u;
    const int b = 4 * gi;
    if (b + 3 < nw) { const sv_u32x4 t = *reinterpret_cast<const sv_u32x4 *>(g + b); v.x = t.x; v.y = t.y; v.z = t.z; v.w = t.w; }
    else if (b < nw) { v.x = g[b]; if (b + 1 < nw) v.y = g[b + 1]; if (b + 2 < nw) v.z = g[b + 2]; }
    return v;
}
static __device__ __forceinline__ void prefetch_read(const DevReads &R, uint64_t r, int lane, ReadPrefetch &pf)
{
    const uint32_t *g = R.packed + rd_word_off(R, r);
    const int L = (int)uni(rd_len(R, r));
    const int nw = (L + 15) >> 4;
#pragma unroll
    for (int i = 0; i < SV_PREFETCH_VEC; i++) pf.v[i] = sv_load_group(g, lane + i * WAVE, nw);
    if (R.pos_hint) {
        const uint64_t *ph = R.pos_hint + rd_hint_off(R, r);
        const int nh = (L + 63) >> 6;
#pragma unroll
        for (int i = 0; i < SV_PREFETCH_HINTS; i++) {
            const int wi = lane + i * WAVE;
            pf.hw[i] = wi < nh ? ph[wi] : 0ull;
        }
    }
    pf.r = r;
}
// the read's per-position hint words into LDS: search_core looks at one of them per seed candidate and scans them for the
// next candidate — as global loads these were some 25 dependent round trips per 10 kbp read
static __device__ void load_hints_to_lds(const DevReads &R, uint64_t r, int L, uint64_t *l_hint, int lane, const ReadPrefetch &pf)
{
    const int nh = (L + 63) >> 6;
    int first = lane;
    if (pf.r == r) {
#pragma unroll
        for (int i = 0; i < SV_PREFETCH_HINTS; i++) {
            const int wi = lane + i * WAVE;
            if (wi < nh) l_hint[wi] = pf.hw[i];
        }
        first = lane + SV_PREFETCH_HINTS * WAVE;
        if (nh <= SV_PREFETCH_HINTS * WAVE) return;      // (wave-uniform: nothing left, and no look-up of the read's offset)
    }
    const uint64_t *ph = R.pos_hint + rd_hint_off(R, r);
    for (int wi = first; wi < nh; wi += WAVE) l_hint[wi] = ph[wi];
}

static __device__ void load_read_to_lds(const DevReads &R, uint64_t r, uint8_t *seq, uint32_t *words, int L, int lane,
                                        const ReadPrefetch *pf = nullptr)
{
    const uint32_t *g = R.packed + rd_word_off(R, r);
    const int nw = (L + 15) >> 4;
    const int ng = (nw + 4) >> 2;                 // groups up to and including the one that holds word nw (= 0: lds_code reads one word past the last)
    const bool have = pf && pf->r == r;           // wave-uniform
    uint4 *w4 = reinterpret_cast<uint4 *>(words);   // (the words' LDS region is 16-byte aligned and a multiple of four words long)
    int first = lane;
    if (have) {
#pragma unroll
        for (int i = 0; i < SV_PREFETCH_VEC; i++) {
            const int gi = lane + i * WAVE;
            if (gi < ng) w4[gi] = pf->v[i];
        }
        first = lane + SV_PREFETCH_VEC * WAVE;
    }
    for (int gi = first; gi < ng; gi += WAVE) w4[gi] = sv_load_group(g, gi, nw);
    (void)seq;                                          // (the ASCII copy: region by region, when a byte-wise consumer is entered — rh_ascii)
}

#define PROF_READ_DONE(cat_, tot_) do { \
            wave_sync(); \
            if (lane == 0) { h.lprof[PF_TOTAL] = (tot_); h.lprof[PF_READS] = 1ull; } \
            wave_sync(); \
            unsigned long long *ws_ = h.lprof + PF_SLOTS + (cat_) * PF_SLOTS; \
            if (lane < PF_SLOTS && lane != PF_MAX) ws_[lane] += h.lprof[lane]; \
            if (lane == PF_MAX && (tot_) > ws_[PF_MAX]) ws_[PF_MAX] = (tot_); \
            if (lane == 0) { int b_ = 63 - __clzll((long long)((tot_) | 1ull)) - 8; b_ = b_ < 0 ? 0 : (b_ >= PF_BINS ? PF_BINS - 1 : b_); h.lprof[5 * PF_SLOTS + (cat_) * PF_BINS + b_] += 1ull; } \
            wave_sync(); } while (0)
#define PROF_WAVE_FLUSH() do { if (h.lprof) { wave_sync(); \
            if (lane == 0) { atomicAdd(P.prof + 190, (unsigned long long)__builtin_readcyclecounter() - wave_c0); atomicAdd(P.prof + 191, (unsigned long long)__builtin_amdgcn_s_memrealtime() - wave_r0); \
                             atomicMax(P.prof + 189, (unsigned long long)__builtin_amdgcn_s_memrealtime()); atomicAdd(P.prof + 186, 1ull); \
                             if (blockIdx.x < 16384) P.prof[193 + 2 * blockIdx.x] = (unsigned long long)__builtin_amdgcn_s_memrealtime(); } \
            for (int q_ = lane; q_ < 4 * PF_SLOTS + 4 * PF_BINS; q_ += WAVE) { \
                const unsigned long long v_ = h.lprof[PF_SLOTS + q_]; \
                if (v_) { if (q_ < 4 * PF_SLOTS && (q_ % PF_SLOTS) == PF_MAX) atomicMax(P.prof + q_, v_); else atomicAdd(P.prof + q_, v_); } } } } while (0)
template <bool EXC>
// (two waves per SIMD asked for, i.e. up to 256 VGPRs: with one wave per block and 14-58 KB of LDS per block the LDS decides
// the residency — and the next read's prefetched words did not fit the 128 registers of a 4-wave target without spilling)
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_survivor(DevReads R, DevParams P, const uint64_t *surv_idx,
                                                   const uint32_t *d_n_surv, uint64_t n_max, SurvOut *out,
                                                   char *dr_chars, uint32_t dr_stride, uint32_t *ss_pool,
                                                   uint32_t ss_pool_cap, uint32_t *d_ss_used,
                                                   uint8_t *found_flag, const uint32_t *seed_hint, SurvLds lds, int punt_only, uint64_t slot_base, uint64_t slot_total,
                                                   const uint32_t *punt_list, const uint32_t *d_punt_n, uint32_t *redo_list)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t sv_lds[];
    const int lane = threadIdx.x;
    RH h;
    h.seq = sv_lds;
    h.seq_buf = sv_lds; h.seq_win = EXC ? 0 : (int)lds.seq_window;
    h.ss = reinterpret_cast<uint32_t *>(sv_lds + lds.seq_bytes);
    h.cap = (int)lds.ss_cap;
    h.rowA = reinterpret_cast<uint16_t *>(h.ss + lds.ss_cap);
    h.rowB = h.rowA + lds.row_elems;
    h.row_cap = (int)lds.row_elems;
    uint32_t *l_words = reinterpret_cast<uint32_t *>(h.rowB + lds.row_elems);
    h.words = EXC ? nullptr : l_words;
    h.sims = reinterpret_cast<float *>(l_words + lds.words_cap);
    uint64_t *l_hint = reinterpret_cast<uint64_t *>(h.sims + lds.ss_cap);
    h.cmask = (1u << (2 * P.window)) - 1u;
    // diagnostics: the launch was given PF_SLOTS x 8 more bytes of LDS behind the layout (launch_survivor)
    h.lprof = P.prof ? reinterpret_cast<unsigned long long *>(sv_lds + ((lds.total_bytes + 7u) & ~7u)) : nullptr;
    if (h.lprof) { for (int q = lane; q < PF_LDS_WORDS; q += WAVE) h.lprof[q] = 0ull; wave_sync(); }
    // (the wave's lifetime on both clocks: s_memtime counts shader cycles, s_memrealtime a constant 100 MHz — their ratio is the
    // clock the launch really ran at; slots 190 / 191 of the counters)
    const unsigned long long wave_c0 = h.lprof ? (unsigned long long)__builtin_readcyclecounter() : 0ull;
    const unsigned long long wave_r0 = h.lprof ? (unsigned long long)__builtin_amdgcn_s_memrealtime() : 0ull;
    if (h.lprof && lane == 0) { atomicMin(P.prof + 188, wave_r0); atomicMax(P.prof + 187, wave_r0); }      // first and last wave START
    if (h.lprof && lane == 0 && blockIdx.x < 16384) P.prof[192 + 2 * blockIdx.x] = wave_r0;
    // EXC with punt_only == 5: exception reads that sit in the survivor list (slot s, read surv_idx[s])
    uint64_t n_surv = (EXC && punt_only != 5) ? R.n_exc : (uint64_t)(*d_n_surv);
    if (n_surv > n_max) n_surv = n_max;
    // punt mode: only the reads an earlier launch handed over (err == punt_only: 4 from the lane kernel, 6 = row buffer).  Each wave looks at 64 slots at once and
    // then walks the (rare) flagged ones, instead of every wave polling its slots one dependent load at a time.
    // ... or, with punt_list, exactly the slots on that list (k_long_light's hand-overs, in any order: every result is addressed by
    // its slot), dealt out one at a time over a grid of resident waves — 64 slots per wave left a wave anything from none to a dozen
    // array reads and the launch took twice its share (3.2 ms for 51 k reads at 10 kbp)
    // (the lane kernel's punts, counted by it: usually none — the scan of every slot's error byte for them was 10-17 us of the step)
    if (!EXC && punt_only == 4 && !punt_list && d_punt_n && *d_punt_n == 0u) { PROF_WAVE_FLUSH(); return; }
    uint64_t punt_base = (uint64_t)blockIdx.x * WAVE, punt_mask = 0;
    uint64_t lp = blockIdx.x;
    const uint64_t n_list = punt_list ? (uint64_t)(*d_punt_n) : 0;
    ReadPrefetch pf;
    pf.r = ~0ull;
    uint64_t next_s = ~0ull, next_r = 0;
    for (uint64_t s = blockIdx.x;; ) {
        if (punt_only && punt_list) {
            if (lp >= n_list) { PROF_WAVE_FLUSH(); return; }
            s = uni(punt_list[lp]);
            lp += gridDim.x;
        } else if (punt_only) {
            while (punt_mask == 0) {
                if (punt_base >= n_surv) { PROF_WAVE_FLUSH(); return; }
                const uint64_t q = punt_base + lane;
                punt_mask = __ballot(q < n_surv && out[q].err == (uint8_t)punt_only);
                if (punt_mask == 0) punt_base += (uint64_t)gridDim.x * WAVE;
            }
            const int b = __ffsll((unsigned long long)punt_mask) - 1;
            punt_mask &= punt_mask - 1;
            s = punt_base + b;
            if (punt_mask == 0) punt_base += (uint64_t)gridDim.x * WAVE;
        } else if (s >= n_surv) { PROF_WAVE_FLUSH(); return; }
        uint64_t r;
        int L;
        wave_sync();
        const unsigned long long prof_t0 = h.lprof ? (unsigned long long)__builtin_readcyclecounter() : 0ull;
        if (h.lprof) { if (lane < PF_SLOTS) h.lprof[lane] = 0ull; wave_sync(); }

        if (EXC) {
            uint64_t e = s;
            if (punt_only == 5) {
                r = uni64(surv_idx[s]);
                uint64_t lo = 0, hi = R.n_exc;                  // exc_read[] is ascending: first entry >= r is r itself
                while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (R.exc_read[mid] < r) lo = mid + 1; else hi = mid; }
                e = lo;
            } else r = uni64(R.exc_read[s]);
            uint64_t o0 = uni64(R.exc_off[e]);
            L = (int)uni((uint32_t)(R.exc_off[e + 1] - o0));
            for (int i = lane; i < L; i += WAVE) h.seq[i] = R.exc_bytes[o0 + i];
        } else {
            // (surv_idx == nullptr: the list is 0, 1, 2, ... — a long-read set without exception reads, every read survives)
            r = (next_s == s) ? next_r : (surv_idx ? uni64(surv_idx[s]) : s + slot_base);    // (the prefetch below already looked it up)
            if (!punt_only && R.n_exc && rd_is_exc(R, r)) {     // left to the exception pass
                if (lane == 0) { SurvOut x; x.found = 0; x.n_ss = 0; x.repeat_len = 0; x.ss_off = 0; x.dr_len = 0; x.low_lexi = 0; x.err = 5; out[s] = x; }
                s += gridDim.x;
                continue;
            }
            L = (int)uni(rd_len(R, r));
            // long reads: a read without a single hinted LATTICE seed (39 % of random 10 kbp reads) never leaves the lattice and
            // searchCore returns false without having looked at a base — neither does this wave (no 10 KB of LDS to fill)
            bool no_seed = false;
            if (R.pos_hint && !punt_only) {
                const int nh = (L + 63) >> 6;
                bool any = false;
                if (pf.r == r) {
#pragma unroll
                    for (int i = 0; i < SV_PREFETCH_HINTS; i++) any |= (lane + i * WAVE < nh) && pf.hw[i] != 0ull;
                    if (nh > SV_PREFETCH_HINTS * WAVE) any = true;                 // (longer than the prefetch covers: walk it)
                } else {
                    const uint64_t *gh = R.pos_hint + rd_hint_off(R, r);
                    for (int wi = lane; wi < nh; wi += WAVE) any |= gh[wi] != 0ull;
                }
                no_seed = __ballot(any) == 0ull;
            }
            if (!no_seed) {
                load_read_to_lds(R, r, h.seq, l_words, L, lane, &pf);
                if (R.pos_hint) load_hints_to_lds(R, r, L, l_hint, lane, pf);
            }
            pf.r = ~0ull;
            if (!punt_only && s + gridDim.x < n_surv) {         // the next read of this wave: its words travel during the search
                const uint64_t r2 = surv_idx ? uni64(surv_idx[s + gridDim.x]) : s + gridDim.x + slot_base;
                next_s = s + gridDim.x; next_r = r2;
                if (!R.n_exc || !rd_is_exc(R, r2)) prefetch_read(R, r2, lane, pf);
            } else if (punt_only && punt_list && lp < n_list) { // (list mode: the slot after this one is known as well)
                const uint64_t s2 = uni(punt_list[lp]);
                const uint64_t r2 = surv_idx ? uni64(surv_idx[s2]) : s2 + slot_base;
                next_s = s2; next_r = r2;
                prefetch_read(R, r2, lane, pf);
            }
            if (no_seed) {
                if (lane == 0) { SurvOut x; x.found = 0; x.n_ss = 0; x.repeat_len = 0; x.ss_off = 0; x.dr_len = 0; x.low_lexi = 0; x.err = 0; out[s] = x; }
                if (h.lprof) { const unsigned long long tot = (unsigned long long)__builtin_readcyclecounter() - prof_t0; PROF_READ_DONE(0, tot); }
                s += gridDim.x;
                continue;
            }
        }
        wave_sync();
        if (h.lprof && lane == 0) h.lprof[PF_STAGE] = (unsigned long long)__builtin_readcyclecounter() - prof_t0;
        h.L = L; h.nss = 0; h.replen = 0; h.err = 0;
        h.asc_lo = 0; h.asc_hi = 0; h.asc_pad = (int)(P.highDR + P.highSp) + 32; h.seq = h.seq_buf;
        const uint32_t hint = (!EXC && seed_hint) ? seed_hint[r] : 0xFFFFFFFFu;
        uint64_t *ph = (!EXC && R.pos_hint) ? l_hint : nullptr;            // (staged in LDS above)
        uint32_t *cls_from = reinterpret_cast<uint32_t *>(l_hint + lds.hint_words - 4);      // (the last four hint slots: 8 x uint32)
        if (ph && lane < 8) cls_from[lane] = (lane == 0 || R.hint_all) ? 0u : 0xFFFFFFFFu;      // (hint_all: every class is there from the start)
        wave_sync();
        // (a read the light walk handed over: on from the seed it stopped at — SurvOut::repeat_len of the slot, k_long_light)
        const uint32_t j_start = (!EXC && punt_only == 7) ? uni(out[s].repeat_len) : 0u;
        int f = (P.debug_stop == 1) ? 0 : search_core(h, P, hint, lane, ph, ph ? cls_from : nullptr, j_start);
        const unsigned long long prof_t1 = h.lprof ? (unsigned long long)__builtin_readcyclecounter() : 0ull;
        SurvOut o;
        o.found = 0; o.n_ss = 0; o.repeat_len = 0; o.ss_off = 0; o.dr_len = 0; o.low_lexi = 0; o.err = 0;
        // (-3: Levenshtein rows too short / the ASCII window too small in this launch's LDS layout; -2 in a layout with a capped
        // start/stop list: the same — the launch with the full layout decides)
        if (f == -3 || (f == -2 && lds.ss_cap < lds.ss_slot)) o.err = 6;
        else if (f < 0) o.err = (f == -2) ? 2 : 1;
        if (f == 1 && P.debug_stop != 4) {
            int low = 0;
            int dlen = dr_low_lexi(h, dr_chars + s * (uint64_t)dr_stride, (int)dr_stride, low, lane);
            if (dlen < 0 || dlen > (int)dr_stride) o.err = 1;
            else {
                // start/stop pool: a fixed slot per survivor when the pool is large enough (short reads),
                // otherwise bump allocation (one contended atomic per found read: long reads only)
                // (slot_base / slot_total: this launch covers the slots [slot_base, slot_base + n) of slot_total — the walk of a
                // long-read set runs slice by slice, `out` and `dr_chars` already point at the slice, the pool is shared)
                uint32_t off = 0;
                if ((slot_total ? slot_total : n_surv) * lds.ss_slot <= ss_pool_cap) off = (uint32_t)(s + slot_base) * lds.ss_slot;
                else {
                    if (lane == 0) off = atomicAdd(d_ss_used, (uint32_t)h.nss);
                    off = (uint32_t)__shfl((int)off, 0);
                }
                if ((uint64_t)off + (uint64_t)h.nss > ss_pool_cap) o.err = 3;
                else {
                    for (int k = lane; k < h.nss; k += WAVE) ss_pool[off + k] = h.ss[k];
                    o.found = 1; o.n_ss = (uint32_t)h.nss; o.repeat_len = (uint32_t)h.replen;
                    o.ss_off = off; o.dr_len = (uint16_t)dlen; o.low_lexi = (uint8_t)low;
                    if (lane == 0) found_flag[rd_header_id(R, r)] = 1;      // readsFound[header] = true (:138)
                }
            }
        }
        if (lane == 0) out[s] = o;
        // (a read this launch's layout cannot hold goes on the list of the launch with the full layout: that launch then visits
        // exactly those slots instead of polling every slot's error byte — 68 us for 1 M slots of which none is flagged)
        if (redo_list && o.err == 6 && lane == 0) redo_list[1u + atomicAdd(redo_list, 1u)] = (uint32_t)s;
        if (h.lprof && lane == 0) h.lprof[PF_OUT] = (unsigned long long)__builtin_readcyclecounter() - prof_t1;
        if (h.lprof) {
            // category 1: walked, nothing found; 2: found; 3: handed over / error (0: skipped, no hinted seed)
            const unsigned long long tot = (unsigned long long)__builtin_readcyclecounter() - prof_t0;
            const int cat = o.err ? 3 : (o.found ? 2 : 1);
            PROF_READ_DONE(cat, tot);
            if (lane == 0) atomicMax(P.prof + 185, (tot << 24) | (unsigned long long)((s + slot_base) & 0xFFFFFFull));      // the slowest read's slot
        }
        if (!punt_only) s += gridDim.x;
    }
}

// ------------------------------------------------------------------------------------
// Long reads, the LIGHT walk.  19 reads in 20 of a long-read set hold no array: their searchCore (libcrispr.cpp:265-395) is a
// walk over ~1 250 seeds of which one or two have a chance copy in range, a two-repeat candidate that the extension rejects, a
// move to another residue class (:390) and more walking.  The full wave kernel above spends 34 k cycles on such a read — all of
// it dependent latency (LDS round trips, fenced list appends, vector arithmetic on wave-uniform values) at three waves per SIMD,
// because it carries the QC, the Levenshtein rows, the ASCII window and a start/stop list for the one read in 20 that needs them.
// This kernel is that walk alone: the read's packed words in LDS (2.5 KB at 10 kbp, nothing else), the CURRENT residue class's
// hint words in registers (lane l: words base + l, base + l + 64, ...; the lattice class from k_hint_positions, any other
// computed here 64 words at a time as the walk reaches them), a candidate's two repeats in scalar registers, the two-repeat
// extension in closed form.  Whatever needs more — a third repeat (an array), a candidate due for qcFoundRepeats, a read beyond
// 12 288 bases, an error path — is HANDED OVER (err = 7) to k_survivor<false>, which redoes that read from its first base with
// the reference's full control flow.  A read that is not handed over is decided here: not found.
// ------------------------------------------------------------------------------------
#define LL_HW 3                                   // hint words per lane: 192 per read = 12 288 bases
#define LL_VEC 3                                  // 16-byte word groups per lane: 768 words
struct LightPrefetch { uint4 v[LL_VEC]; uint64_t hw[LL_HW]; };

static __device__ __forceinline__ void ll_prefetch(const DevReads &R, uint64_t r, int lane, LightPrefetch &pf)
{
    const uint32_t *g = R.packed + rd_word_off(R, r);
    const int L = (int)uni(rd_len(R, r));
    const int nw = (L + 15) >> 4, nh = (L + 63) >> 6;
#pragma unroll
    for (int i = 0; i < LL_VEC; i++) pf.v[i] = sv_load_group(g, lane + i * WAVE, nw);
    const uint64_t *ph = R.pos_hint + rd_hint_off(R, r);
#pragma unroll
    for (int i = 0; i < LL_HW; i++) { const int wi = lane + i * WAVE; pf.hw[i] = wi < nh ? ph[wi] : 0ull; }
}

// first hinted position >= j among the hint words held in registers (word cur_base + lane + 64 i in cur[i], the first `done`
// words valid), 0xFFFFFFFF if none
static __device__ __forceinline__ uint32_t ll_next_hinted(const uint64_t (&cur)[LL_HW], uint32_t cur_base, uint32_t done, uint32_t j, int lane)
{
    const uint32_t jw = j >> 6;
#pragma unroll
    for (int i = 0; i < LL_HW; i++) {
        if (64u * (uint32_t)i >= done) break;                                   // (wave-uniform)
        if (cur_base + 64u * (uint32_t)i + 63u < jw) continue;
        const uint32_t t = cur_base + 64u * (uint32_t)i + (uint32_t)lane;
        uint64_t m = (64u * (uint32_t)i + (uint32_t)lane < done) ? cur[i] : 0ull;
        if (t < jw) m = 0ull;
        else if (t == jw) m &= ~0ull << (j & 63u);
        const uint64_t b = __ballot(m != 0ull);
        if (b) {
            const int l0 = __ffsll((unsigned long long)b) - 1;
            const uint64_t mm = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(m >> 32), l0) << 32) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)m, l0);
            return (cur_base + 64u * (uint32_t)i + (uint32_t)l0) * 64u + (uint32_t)(__ffsll((unsigned long long)mm) - 1);
        }
    }
    return 0xFFFFFFFFu;
}

template <bool RANGE>
// surv_idx (optional): slot s holds read surv_idx[s] — the dense path's survivor list (reads of 513 .. 2 048 bases, whose
// survivors the lane kernel does not take: until round 6 every one of them was a walk of the full wave kernel); nullptr: s + slot_base
__global__ __launch_bounds__(WAVE) void k_long_light(DevReads R, DevParams P, const uint32_t *d_n, uint64_t n_max, SurvOut *out, uint64_t slot_base,
                                                     uint32_t *punt_list, uint32_t *d_punt_n, const uint64_t *surv_idx)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t ll_words[];
    const int lane = threadIdx.x;
    uint64_t n = (uint64_t)(*d_n);
    if (n > n_max) n = n_max;
    const uint32_t cmask = (1u << (2 * P.window)) - 1u;
    const int w = (int)P.window;
    LightPrefetch pf;
    auto read_of = [&](uint64_t sl) -> uint64_t { return surv_idx ? uni64(surv_idx[sl]) : sl + slot_base; };
    if (blockIdx.x < n) ll_prefetch(R, read_of(blockIdx.x), lane, pf);
    for (uint64_t s = blockIdx.x; s < n; s += gridDim.x) {
        const uint64_t r = read_of(s);
        if (surv_idx && R.n_exc && rd_is_exc(R, r)) {                             // an exception read in the list: left to the exception pass
            if (lane == 0) { SurvOut x; x.found = 0; x.n_ss = 0; x.repeat_len = 0; x.ss_off = 0; x.dr_len = 0; x.low_lexi = 0; x.err = 5; out[s] = x; }
            if (s + gridDim.x < n) ll_prefetch(R, read_of(s + gridDim.x), lane, pf);
            continue;
        }
        const int L = (int)uni(rd_len(R, r));
        const int nw = (L + 15) >> 4, nh = (L + 63) >> 6;
        uint64_t cur[LL_HW];
        bool any = false;
#pragma unroll
        for (int i = 0; i < LL_HW; i++) { cur[i] = pf.hw[i]; any |= cur[i] != 0ull; }
        const bool too_long = nh > LL_HW * WAVE;
        const bool seeds = __ballot(any) != 0ull;
        uint8_t verdict = 0;                                                     // 0: searchCore returns false; 7: handed over
        uint32_t punt_j = 0;                                                     // ... from this seed on (the iterations before it are done)
        if (too_long) verdict = 7;
        wave_sync();                                                             // (the previous read's LDS accesses are done)
        if (seeds && !too_long) {
            const int ng = (nw + 4) >> 2;                                        // groups up to the one that holds word nw (= 0)
            uint4 *w4 = reinterpret_cast<uint4 *>(ll_words);
#pragma unroll
            for (int i = 0; i < LL_VEC; i++) { const int gi = lane + i * WAVE; if (gi < ng) w4[gi] = pf.v[i]; }
        }
        if (s + gridDim.x < n) ll_prefetch(R, read_of(s + gridDim.x), lane, pf);  // the next read travels during this one's walk
        if (seeds && !too_long) {
            wave_sync();
            const uint32_t seq_length = (uint32_t)L;
            const int searchEnd = (int)(seq_length - P.lowDR - P.lowSp - P.window - 1);
            uint32_t j = 0, rho = 0, cur_base = 0, done = (uint32_t)nh;          // the lattice class: every word is there
            const uint32_t n_hw = searchEnd >= 0 ? ((uint32_t)searchEnd >> 6) + 1u : 0u;      // hint words that hold a seed
            while (searchEnd >= 0 && j <= (uint32_t)searchEnd) {
                j = uni(j); rho = uni(rho); cur_base = uni(cur_base); done = uni(done);
                // the class's hint words are computed 64 at a time, when the walk gets there (a class is left again after
                // 4 000 bases one time in three: most of a class's words would never be looked at)
                uint32_t p = ll_next_hinted(cur, cur_base, done, j, lane);
                while (p == 0xFFFFFFFFu && cur_base + done < n_hw && done < 64u * LL_HW) {
                    const uint32_t t = cur_base + done + (uint32_t)lane;
                    uint64_t bits = 0ull;
                    if (t < (uint32_t)nh) {
                        uint32_t ww[13];
#pragma unroll
                        for (int i = 0; i < 13; i++) { const uint32_t wi = 4u * t + (uint32_t)i; ww[i] = wi < (uint32_t)nw ? ll_words[wi] : 0u; }
                        bits = hint_bits_any<RANGE>(ww, rho, (int)(P.lowDR + P.lowSp), (int)(P.highDR + P.highSp));
                    }
                    const uint32_t round = done >> 6;
#pragma unroll
                    for (int i = 0; i < LL_HW; i++) if ((uint32_t)i == round) cur[i] = bits;
                    done += 64u;
                    p = ll_next_hinted(cur, cur_base, done, j, lane);
                }
                if (p == 0xFFFFFFFFu || p > (uint32_t)searchEnd) break;         // no seed left: false
                j = p;
                uint32_t beginSearch = j + P.lowDR + P.lowSp;
                uint32_t endSearch = j + P.highDR + P.highSp + P.window;
                if (endSearch >= seq_length) endSearch = seq_length - 1;
                if (endSearch < beginSearch) endSearch = beginSearch;
                if (beginSearch > seq_length) { verdict = 7; punt_j = j; break; }   // (the reference throws here: the full kernel reports it)
                const int pos = uni(wave_find_packed(ll_words, cmask, (int)beginSearch, (int)endSearch, (int)j, w, lane));
                if (pos < 0) { j += P.skips; continue; }                         // (the hints are a superset)
                // two repeats at j and pos.  scanRight's first link (libcrispr.cpp:170-263): a third repeat means an array
                {
                    const uint32_t last = (uint32_t)pos, spacing = last - j;
                    const int cand = (int)(last + spacing);
                    uint32_t b3 = (uint32_t)cand - 24u, e3 = (uint32_t)cand + (uint32_t)w + 24u;
                    const uint32_t minb = last + (uint32_t)w + P.lowSp;
                    if (b3 < minb) b3 = minb;
                    if (b3 <= seq_length - 1) {
                        if (e3 > seq_length) e3 = seq_length;
                        if (b3 < e3 && wave_find_packed(ll_words, cmask, (int)b3, (int)e3, (int)j, w, lane) >= 0) { verdict = 7; punt_j = j; break; }
                    }
                }
                if (2u < P.minRepeats) { j += P.skips; continue; }               // (-n 3 and up: two repeats are not a candidate)
                // extendPreRepeat for two repeats, closed form (extend_pre_repeat_packed / ln_extend2)
                uint32_t right, left;
                {
                    const int jj = (int)j, pp = pos, spacing = pp - jj;
                    int max_right = spacing - (int)P.lowSp;
                    if (max_right > L - (pp + w)) max_right = L - (pp + w);
                    int rr = 0;
                    while (rr < max_right) {
                        uint64_t a0, a1, b0, b1;
                        wv_load128(ll_words, jj + w + rr, a0, a1); wv_load128(ll_words, pp + w + rr, b0, b1);
                        const int nn = max_right - rr < 64 ? max_right - rr : 64;
                        const int q = uni(ln_run_up(a0 ^ b0, a1 ^ b1, nn));
                        rr += q;
                        if (q < nn) break;
                    }
                    int max_left = spacing - (w + rr);
                    if (max_left < 0) max_left = 0;
                    if (max_left > jj) max_left = jj;
                    int ll = 0;
                    while (ll < max_left) {
                        const int nn = max_left - ll < 64 ? max_left - ll : 64;
                        uint64_t a0, a1, b0, b1;
                        wv_load128(ll_words, jj - ll - nn, a0, a1); wv_load128(ll_words, pp - ll - nn, b0, b1);
                        const int q = uni(ln_run_down(a0 ^ b0, a1 ^ b1, nn));
                        ll += q;
                        if (q < nn) break;
                    }
                    right = (uint32_t)rr; left = (uint32_t)ll;
                }
                const uint32_t replen = (uint32_t)w + right + left;
                if (replen >= P.lowDR && replen <= P.highDR) { verdict = 7; punt_j = j; break; }          // due for qcFoundRepeats
                // rejected: on behind the last repeat's (extended, clamped) end (:390)
                uint32_t last_end = (uint32_t)pos + (uint32_t)w - 1u;
                if (last_end >= seq_length) last_end = seq_length - 1;                       // (startStopsAdd's clamp)
                last_end = (last_end + right >= seq_length) ? seq_length - 1 : last_end + right;
                j = last_end - 1u + P.skips;
                if ((j & 7u) != rho) { rho = j & 7u; cur_base = j >> 6; done = 0u; }
            }
        }
        if (lane == 0) {
            SurvOut x; x.found = 0; x.n_ss = 0; x.repeat_len = punt_j; x.ss_off = 0; x.dr_len = 0; x.low_lexi = 0; x.err = verdict; out[s] = x;
            if (verdict == 7) punt_list[atomicAdd(d_punt_n, 1u)] = (uint32_t)(s + slot_base);     // (the slot in the whole set's numbering)
        }
    }
}

// ---- the light walk for ANY window and seed lattice (-w / -d on long reads) ----
// The hint forms above know one residue class mod 8 at a time; with another lattice (skips = lowDR - 2 w + 1) or window the
// every-position form of the scan (k_filter_fast_any) gives ONE bit per base — "the w-mer here has a copy D0 .. D1 further on" —
// for whatever lattice the walk is on, so there is no class to switch: the walking wave computes the bits of the next 64 hint words
// when it gets there (lane = hint word: 4 packed words + halo, 11 instructions per word and shift), finds the next set bit at or
// behind j and takes it if it lies on the lattice that starts at j.  No hint kernel, no hint array.  Everything else is
// k_long_light.  (1 M x 10 kbp with -d 20 -D 40: 512 ms on the un-hinted wave kernel.)
__global__ __launch_bounds__(WAVE) void k_long_light_any(DevReads R, DevParams P, const uint32_t *d_n, uint64_t n_max, SurvOut *out, uint64_t slot_base,
                                                         uint32_t *punt_list, uint32_t *d_punt_n, const uint64_t *surv_idx)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t ll_words[];
    const int lane = threadIdx.x;
    uint64_t n = (uint64_t)(*d_n);
    if (n > n_max) n = n_max;
    const uint32_t cmask = (1u << (2 * P.window)) - 1u;
    const int w = (int)P.window;
    const int D0 = (int)(P.lowDR + P.lowSp), D1 = (int)(P.highDR + P.highSp);
    uint4 pfv[LL_VEC];
    auto prefetch = [&](uint64_t r) {
        const uint32_t *g = R.packed + rd_word_off(R, r);
        const int nw = ((int)uni(rd_len(R, r)) + 15) >> 4;
#pragma unroll
        for (int i = 0; i < LL_VEC; i++) pfv[i] = sv_load_group(g, lane + i * WAVE, nw);
    };
    auto read_of = [&](uint64_t sl) -> uint64_t { return surv_idx ? uni64(surv_idx[sl]) : sl + slot_base; };
    if (blockIdx.x < n) prefetch(read_of(blockIdx.x));
    for (uint64_t s = blockIdx.x; s < n; s += gridDim.x) {
        const uint64_t r = read_of(s);
        if (surv_idx && R.n_exc && rd_is_exc(R, r)) {                             // an exception read in the list: left to the exception pass
            if (lane == 0) { SurvOut x; x.found = 0; x.n_ss = 0; x.repeat_len = 0; x.ss_off = 0; x.dr_len = 0; x.low_lexi = 0; x.err = 5; out[s] = x; }
            if (s + gridDim.x < n) prefetch(read_of(s + gridDim.x));
            continue;
        }
        const int L = (int)uni(rd_len(R, r));
        const int nw = (L + 15) >> 4, nh = (L + 63) >> 6;
        const bool too_long = nh > LL_HW * WAVE;
        uint8_t verdict = too_long ? 7 : 0;
        uint32_t punt_j = 0;
        wave_sync();
        if (!too_long) {
            const int ng = (nw + 4) >> 2;
            uint4 *w4 = reinterpret_cast<uint4 *>(ll_words);
#pragma unroll
            for (int i = 0; i < LL_VEC; i++) { const int gi = lane + i * WAVE; if (gi < ng) w4[gi] = pfv[i]; }
        }
        if (s + gridDim.x < n) prefetch(read_of(s + gridDim.x));
        if (!too_long) {
            wave_sync();
            const uint32_t seq_length = (uint32_t)L;
            const int searchEnd = (int)(seq_length - P.lowDR - P.lowSp - P.window - 1);
            const uint32_t n_hw = searchEnd >= 0 ? ((uint32_t)searchEnd >> 6) + 1u : 0u;
            uint64_t cur[LL_HW] = {};
            const uint64_t *stored = (R.pos_hint && R.hint_all) ? R.pos_hint + rd_hint_off(R, r) : nullptr;
            uint32_t j = 0, done = 0, from = 0;          // `from`: the next position to look at (>= j); seeds are j, j + skips, ...
            while (searchEnd >= 0 && j <= (uint32_t)searchEnd) {
                j = uni(j); done = uni(done); from = uni(from);
                uint32_t p = ll_next_hinted(cur, 0u, done, from, lane);
                while (p == 0xFFFFFFFFu && done < n_hw && done < 64u * LL_HW) {
                    const uint32_t t = done + (uint32_t)lane;
                    uint64_t bits = 0ull;
                    if (t < (uint32_t)nh) {
                        if (stored) bits = stored[t];              // (every position's bit is there already: k_hint_filter_any kept them, DevReads.hint_all)
                        else {
                            uint32_t ww[13];
#pragma unroll
                            for (int i = 0; i < 13; i++) { const uint32_t wi = 4u * t + (uint32_t)i; ww[i] = wi < (uint32_t)nw ? ll_words[wi] : 0u; }
                            bits = hint_bits_every(ww, w, D0, D1);
                        }
                    }
                    const uint32_t round = done >> 6;
#pragma unroll
                    for (int i = 0; i < LL_HW; i++) if ((uint32_t)i == round) cur[i] = bits;
                    done += 64u;
                    p = ll_next_hinted(cur, 0u, done, from, lane);
                }
                if (p == 0xFFFFFFFFu || p > (uint32_t)searchEnd) break;
                if ((p - j) % P.skips != 0u) { from = p + 1u; continue; }       // a copy exists there, but it is no seed of this lattice
                j = p;
                uint32_t beginSearch = j + P.lowDR + P.lowSp;
                uint32_t endSearch = j + P.highDR + P.highSp + P.window;
                if (endSearch >= seq_length) endSearch = seq_length - 1;
                if (endSearch < beginSearch) endSearch = beginSearch;
                if (beginSearch > seq_length) { verdict = 7; punt_j = j; break; }
                const int pos = uni(wave_find_packed(ll_words, cmask, (int)beginSearch, (int)endSearch, (int)j, w, lane));
                if (pos < 0) { j += P.skips; from = j; continue; }
                {
                    const uint32_t last = (uint32_t)pos, spacing = last - j;
                    const int cand = (int)(last + spacing);
                    uint32_t b3 = (uint32_t)cand - 24u, e3 = (uint32_t)cand + (uint32_t)w + 24u;
                    const uint32_t minb = last + (uint32_t)w + P.lowSp;
                    if (b3 < minb) b3 = minb;
                    if (b3 <= seq_length - 1) {
                        if (e3 > seq_length) e3 = seq_length;
                        if (b3 < e3 && wave_find_packed(ll_words, cmask, (int)b3, (int)e3, (int)j, w, lane) >= 0) { verdict = 7; punt_j = j; break; }
                    }
                }
                if (2u < P.minRepeats) { j += P.skips; from = j; continue; }
                uint32_t right, left;
                {
                    const int jj = (int)j, pp = pos, spacing = pp - jj;
                    int max_right = spacing - (int)P.lowSp;
                    if (max_right > L - (pp + w)) max_right = L - (pp + w);
                    int rr = 0;
                    while (rr < max_right) {
                        uint64_t a0, a1, b0, b1;
                        wv_load128(ll_words, jj + w + rr, a0, a1); wv_load128(ll_words, pp + w + rr, b0, b1);
                        const int nn = max_right - rr < 64 ? max_right - rr : 64;
                        const int q = uni(ln_run_up(a0 ^ b0, a1 ^ b1, nn));
                        rr += q;
                        if (q < nn) break;
                    }
                    int max_left = spacing - (w + rr);
                    if (max_left < 0) max_left = 0;
                    if (max_left > jj) max_left = jj;
                    int ll = 0;
                    while (ll < max_left) {
                        const int nn = max_left - ll < 64 ? max_left - ll : 64;
                        uint64_t a0, a1, b0, b1;
                        wv_load128(ll_words, jj - ll - nn, a0, a1); wv_load128(ll_words, pp - ll - nn, b0, b1);
                        const int q = uni(ln_run_down(a0 ^ b0, a1 ^ b1, nn));
                        ll += q;
                        if (q < nn) break;
                    }
                    right = (uint32_t)rr; left = (uint32_t)ll;
                }
                const uint32_t replen = (uint32_t)w + right + left;
                if (replen >= P.lowDR && replen <= P.highDR) { verdict = 7; punt_j = j; break; }
                uint32_t last_end = (uint32_t)pos + (uint32_t)w - 1u;
                if (last_end >= seq_length) last_end = seq_length - 1;
                last_end = (last_end + right >= seq_length) ? seq_length - 1 : last_end + right;
                j = last_end - 1u + P.skips;
                from = j;
            }
        }
        if (lane == 0) {
            SurvOut x; x.found = 0; x.n_ss = 0; x.repeat_len = punt_j; x.ss_off = 0; x.dr_len = 0; x.low_lexi = 0; x.err = verdict; out[s] = x;
            if (verdict == 7) punt_list[atomicAdd(d_punt_n, 1u)] = (uint32_t)(s + slot_base);
        }
    }
}

hipError_t launch_long_light(const DevReads &R, const DevParams &P, const uint32_t *d_n, uint64_t n_max, SurvOut *out, uint64_t slot_base,
                             uint32_t max_len, hipStream_t st, uint32_t *punt_list, uint32_t *d_punt_n, const uint64_t *surv_idx)
{
    if (n_max == 0) return hipSuccess;
    const uint32_t words_cap = (((max_len + 15) / 16 + 2) + 3u) & ~3u;
    const uint32_t lds_bytes = (words_cap + 16u) * 4u;                           // (+ the words a 128-base piece reads past the read's last)
    const int grid = (int)std::min<uint64_t>(n_max, 256 * 32);
    if (!R.pos_hint || R.hint_all) {
        // no position hints of the default lattice: another window or seed lattice — the every-position form, hints computed by the
        // walking wave (or read, where the filter kept every position's bit: hint_all)
        if (P.window < 6 || P.window > 9 || P.skips < 1 || P.lowDR + P.lowSp < 17 || P.highDR + P.highSp > 127 || P.highDR + P.highSp < P.lowDR + P.lowSp) return hipErrorNotSupported;
        hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_long_light_any), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e2 != hipSuccess) return e2;
        CRASS_LAUNCH(k_long_light_any, dim3(grid), dim3(WAVE), lds_bytes, st, R, P, d_n, n_max, out, slot_base, punt_list, d_punt_n, surv_idx);
        return hipGetLastError();
    }
    if (P.skips != 8 || P.window != 8) return hipErrorNotSupported;
    static const int force_ll = getenv("CRASS_HINT_RANGE") ? atoi(getenv("CRASS_HINT_RANGE")) : 0;
    const bool range = P.lowDR + P.lowSp != 49 || P.highDR + P.highSp != 97 || (force_ll & 2);
    hipError_t e = hipFuncSetAttribute(range ? reinterpret_cast<const void *>(&k_long_light<true>) : reinterpret_cast<const void *>(&k_long_light<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    if (range) CRASS_LAUNCH(k_long_light<true>, dim3(grid), dim3(WAVE), lds_bytes, st, R, P, d_n, n_max, out, slot_base, punt_list, d_punt_n, surv_idx);
    else CRASS_LAUNCH(k_long_light<false>, dim3(grid), dim3(WAVE), lds_bytes, st, R, P, d_n, n_max, out, slot_base, punt_list, d_punt_n, surv_idx);
    return hipGetLastError();
}


// ------------------------------------------------------------------------------------
// pass 1, step 2 (fast path): the same searchCore, one read per LANE.
//
// The wave-per-read kernel above spends most of its issue slots with one or two useful lanes
// (a serial DP, a serial column vote).  For short packed reads every lane can instead run the
// complete reference control flow for its own read: 64 reads advance together and loops of
// different length simply mask lanes off.  Per-lane state lives in LDS, word-/entry-interleaved
// across lanes ([index][lane]) so that lanes working at the same index hit different banks.
// Anything unusual (string pair with both lengths > 64, start/stop list overflow) is PUNTED
// (err = 4) to the wave-per-read kernel, which re-runs that read from scratch.
// Semantics are line-for-line those of search_core()/oracle; the parity suites cover both.
// ------------------------------------------------------------------------------------
struct LaneRead {
    const uint32_t *w;      // LDS: word i of this lane's read at w[i * 64]
    uint16_t *ss;           // LDS: start/stop entry k at ss[k * 64]
    int L, nss, cap, replen;
    uint32_t cmask;
    int punt;
};

static __device__ __forceinline__ uint32_t ln_word(const LaneRead &h, int i) { return h.w[i * WAVE]; }
static __device__ __forceinline__ uint32_t ln_base(const LaneRead &h, int p) { return (ln_word(h, p >> 4) >> ((p & 15) * 2)) & 3u; }
static __device__ __forceinline__ uint32_t ln_code(const LaneRead &h, int p)
{
    const int wi = p >> 4, sh = (p & 15) * 2;
    const uint64_t v = ((uint64_t)ln_word(h, wi + 1) << 32) | ln_word(h, wi);
    return (uint32_t)(v >> sh) & h.cmask;
}
static __device__ __forceinline__ uint32_t ln_ss(const LaneRead &h, int k) { return h.ss[k * WAVE]; }
static __device__ __forceinline__ void ln_ss_set(LaneRead &h, int k, uint32_t v) { h.ss[k * WAVE] = (uint16_t)v; }

// bases [start, start + 64) of the lane's read as two 64-bit words (2 bits per base, base `start` in bits 0-1); bases past
// the stored words read as 0.  Five independent LDS reads and four funnel shifts: the loops that follow run on registers
// (a per-base ln_base() in a dependent loop is one LDS round trip per iteration: the QC stage was 82 us of 155 that way).
static __device__ __forceinline__ void ln_load128(const LaneRead &h, int start, uint64_t &lo, uint64_t &hi)
{
    const int wi = start >> 4;
    const uint32_t sh = (uint32_t)(start & 15) * 2u;
    const uint32_t a0 = ln_word(h, wi), a1 = ln_word(h, wi + 1), a2 = ln_word(h, wi + 2), a3 = ln_word(h, wi + 3), a4 = ln_word(h, wi + 4);
    const uint32_t y0 = __builtin_amdgcn_alignbit(a1, a0, sh), y1 = __builtin_amdgcn_alignbit(a2, a1, sh);
    const uint32_t y2 = __builtin_amdgcn_alignbit(a3, a2, sh), y3 = __builtin_amdgcn_alignbit(a4, a3, sh);
    lo = (uint64_t)y0 | ((uint64_t)y1 << 32); hi = (uint64_t)y2 | ((uint64_t)y3 << 32);
}
// even bits of a 64-bit word compacted into the low 32 bits
static __device__ __forceinline__ uint32_t ln_even_bits(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}
// the two bit planes of n <= 64 bases held in (lo, hi): bit i of p0 / p1 = low / high bit of base i
static __device__ __forceinline__ void ln_planes(uint64_t lo, uint64_t hi, int n, uint64_t &p0, uint64_t &p1)
{
    p0 = (uint64_t)ln_even_bits(lo) | ((uint64_t)ln_even_bits(hi) << 32);
    p1 = (uint64_t)ln_even_bits(lo >> 1) | ((uint64_t)ln_even_bits(hi >> 1) << 32);
    const uint64_t m = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    p0 &= m; p1 &= m;
}

// bmpSearch semantics (PatternMatcher.cpp:26-59) for the w-mer at `pat` in [begin, end), one candidate per iteration.  The
// text is pulled through a 64-bit register, 32 bases per refill: no LDS access inside the compare loop (a per-base ln_base()
// there was one LDS round trip per iteration).  The route of -w 9 (18 bits: no two codes per register) and of
// CRASS_LANE_FIND_SERIAL=1, the A/B switch of the packed form below.
static __device__ __noinline__ int ln_find_serial(const uint32_t *w, uint32_t cmask, int begin, int end, int pat, int plen)
{
    LaneRead h;
    h.w = w; h.cmask = cmask;
    if (end - begin <= 0 || plen <= 0 || plen > end - begin) return -1;
    const uint32_t sj = ln_code(h, pat);
    uint32_t code = ln_code(h, begin);
    const int top = 2 * (plen - 1);
    int nb = begin + plen;                               // next base to shift in
    uint64_t buf = 0; int left = 0;                      // bases nb .. nb + left - 1, base nb in bits 0-1
    for (int p = begin;; p++) {
        if (code == sj) return p;
        if (p + 1 + plen > end) return -1;
        if (left == 0) {
            const int wi = nb >> 4;
            const uint32_t sh = (uint32_t)(nb & 15) * 2u;
            const uint32_t a0 = ln_word(h, wi), a1 = ln_word(h, wi + 1), a2 = ln_word(h, wi + 2);
            buf = (uint64_t)__builtin_amdgcn_alignbit(a1, a0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(a2, a1, sh) << 32);
            left = 32;
        }
        code = (code >> 2) | ((uint32_t)(buf & 3ull) << top);
        buf >>= 2; left--; nb++;
    }
}

// The same rule on packed registers (lane_find.h).  The text from `begin` on is brought into four words once
// (ln_load128).  Every pair of candidates t, t + 8 is then one funnel shift at a STATIC amount, one xor-and-mask
// against the duplicated code and two packed 16-bit operations that keep the first match: four instructions per two
// candidates.  The loop above spends 26 per candidate, half of them exec-mask bookkeeping, and a wave runs it for
// as long as its slowest lane, in practice the whole window.
// The candidates are begin .. end - plen: the last one at p + plen <= end, the reference's off-by-one at a clipped
// endSearch = L - 1 included.  A window beyond 64 - plen + 1 candidates (-s / -S / -D) takes several chunks under a
// wave-uniform loop.  serial and plen are the same in every lane.
static __device__ __forceinline__ int ln_find(const LaneRead &h, int begin, int end, int pat, int plen, uint32_t serial)
{
    if (serial || plen > 8) return ln_find_serial(h.w, h.cmask, begin, end, pat, plen);
    int left = (end - begin <= 0 || plen <= 0 || plen > end - begin) ? 0 : end - plen - begin + 1;      // candidates not looked at yet
    const uint32_t sj = ln_code(h, pat);
    const int chunk = 64 - plen + 1;
    int found = -1;
    while (__any((int)(left > 0))) {
        uint64_t lo, hi;
        ln_load128(h, begin, lo, hi);
        const int n = left < chunk ? left : chunk;
        const int t = find_packed_steps(lo, hi, sj, plen, n, __any((int)(n > kLaneFindShortNpos)) != 0);
        if (t >= 0) { found = begin + t; left = 0; }
        else if (left > chunk) { left -= chunk; begin += chunk; }
        else left = 0;
    }
    return found;
}

static __device__ void ln_add(LaneRead &h, uint32_t i, uint32_t j)          // startStopsAdd, ReadHolder.cpp:263-297
{
    if (h.nss + 2 > h.cap) { h.punt = 1; return; }
    if (j >= (uint32_t)h.L) j = (uint32_t)h.L - 1;
    ln_ss_set(h, h.nss, i); ln_ss_set(h, h.nss + 1, j);
    h.nss += 2;
}

static __device__ void ln_scan_right(LaneRead &h, int pat, uint32_t pattern_length, uint32_t minSpacerLength, uint32_t scanRange, uint32_t find_serial)
{   // scanRight, libcrispr.cpp:170-263
    uint32_t last_repeat_index = ln_ss(h, h.nss - 2);
    uint32_t second_last_repeat_index = ln_ss(h, h.nss - 4);
    uint32_t repeat_spacing = last_repeat_index - second_last_repeat_index;
    const uint32_t read_length = (uint32_t)h.L;
    for (;;) {
        int candidate_repeat_index = (int)(last_repeat_index + repeat_spacing);
        uint32_t begin_search = (uint32_t)candidate_repeat_index - scanRange;
        uint32_t end_search = (uint32_t)candidate_repeat_index + pattern_length + scanRange;
        uint32_t scanRightMinBegin = last_repeat_index + pattern_length + minSpacerLength;
        if (begin_search < scanRightMinBegin) begin_search = scanRightMinBegin;
        if (begin_search > read_length - 1) return;
        if (end_search > read_length) end_search = read_length;
        if (begin_search >= end_search) return;
        int position = ln_find(h, (int)begin_search, (int)end_search, pat, (int)pattern_length, find_serial);
        if (position < 0) return;
        ln_add(h, (uint32_t)position, (uint32_t)position + pattern_length - 1);
        if (h.punt) return;
        second_last_repeat_index = last_repeat_index;
        last_repeat_index = (uint32_t)position;
        repeat_spacing = last_repeat_index - second_last_repeat_index;
        if (repeat_spacing < (minSpacerLength + pattern_length)) return;
    }
}

// number of leading equal 2-bit groups of two strings given as xor (x0 low): up to n <= 64 groups
static __device__ __forceinline__ int ln_run_up(uint64_t x0, uint64_t x1, int n)
{
    int r = x0 ? (__ffsll((unsigned long long)x0) - 1) >> 1 : (x1 ? 32 + ((__ffsll((unsigned long long)x1) - 1) >> 1) : 64);
    return r < n ? r : n;
}
// ... of trailing equal groups, counted from group n - 1 downwards (n <= 64, n >= 1)
static __device__ __forceinline__ int ln_run_down(uint64_t x0, uint64_t x1, int n)
{
    int r;
    if (n <= 32) { const uint64_t y = x0 << (64 - 2 * n); r = y ? __clzll((long long)y) >> 1 : n; }
    else {
        const uint64_t y1 = x1 << (64 - 2 * (n - 32));
        if (y1) r = __clzll((long long)y1) >> 1;
        else r = (n - 32) + (x0 ? __clzll((long long)x0) >> 1 : 32);
    }
    return r < n ? r : n;
}

// extendPreRepeat (libcrispr.cpp:520-772) for exactly TWO repeats, in closed form.  With two repeats cut_off = 2 (:538-544),
// so a column is accepted iff both copies hold the same base (:617-651; packed reads hold A/C/G/T only), the right phase
// stops at the first disagreement, after shortest_spacing - minSpacer columns (:581), or when the second copy runs into
// the read end — there the reference drops the last repeat from the vote (:614-616) and the one that is left cannot reach
// the cut-off —; the left phase likewise, bounded by shortest_spacing - length so far (:674-675) and by the read start
// (:700-704).  The agreeing runs are xor + count-zeros on 128-bit pieces of the read instead of a per-column vote.
static __device__ uint32_t ln_extend2(LaneRead &h, int searchWindowLength, int minSpacerLength)
{
    const int j = (int)ln_ss(h, 0), p = (int)ln_ss(h, 2), L = h.L, w = searchWindowLength;
    const int spacing = p - j;
    int max_right = spacing - minSpacerLength;                  // (unsigned in the reference; spacing >= minSpacer + w here)
    if (max_right > L - (p + w)) max_right = L - (p + w);       // the second copy's column must lie inside the read
    int right = 0;
    while (right < max_right) {
        uint64_t a0, a1, b0, b1;
        ln_load128(h, j + w + right, a0, a1); ln_load128(h, p + w + right, b0, b1);
        const int n = max_right - right < 64 ? max_right - right : 64;
        const int r = ln_run_up(a0 ^ b0, a1 ^ b1, n);
        right += r;
        if (r < n) break;
    }
    const int len_r = w + right;
    int max_left = spacing - len_r;
    if (max_left < 0) max_left = 0;
    if (max_left > j) max_left = j;                             // the first copy's column must lie inside the read
    int left = 0;
    while (left < max_left) {
        const int n = max_left - left < 64 ? max_left - left : 64;
        uint64_t a0, a1, b0, b1;
        ln_load128(h, j - left - n, a0, a1); ln_load128(h, p - left - n, b0, b1);
        const int r = ln_run_down(a0 ^ b0, a1 ^ b1, n);
        left += r;
        if (r < n) break;
    }
    h.replen = w + right + left;
    for (int r = 0; r + 1 < h.nss; r += 2) {
        uint32_t a = ln_ss(h, r), b = ln_ss(h, r + 1);
        a = (a < (uint32_t)left) ? 0 : a - (uint32_t)left;
        b = (b + (uint32_t)right >= (uint32_t)L) ? (uint32_t)L - 1 : b + (uint32_t)right;
        ln_ss_set(h, r, a); ln_ss_set(h, r + 1, b);
    }
    return (uint32_t)h.replen;
}

static __device__ uint32_t ln_extend(LaneRead &h, int searchWindowLength, int minSpacerLength)
{   // extendPreRepeat, libcrispr.cpp:520-772 (serial columns, like the reference)
    if (h.nss == 4) return ln_extend2(h, searchWindowLength, minSpacerLength);
    const uint32_t num_repeats = (uint32_t)h.nss / 2;
    h.replen = searchWindowLength;
    int cut_off = (int)(num_repeats - 1);
    if (2 > cut_off) cut_off = 2;
    const uint32_t first_repeat_start_index = ln_ss(h, 0);
    const uint32_t last_repeat_start_index = ln_ss(h, h.nss - 2);
    const uint32_t end_index = (uint32_t)h.nss;
    const uint32_t seqlen = (uint32_t)h.L;
    uint32_t shortest_repeat_spacing = (uint32_t)((int)ln_ss(h, 2) - (int)ln_ss(h, 0));
    for (uint32_t i = 4; i < end_index; i += 2) {
        uint32_t sp = (uint32_t)((int)ln_ss(h, i) - (int)ln_ss(h, i - 2));
        if (sp < shortest_repeat_spacing) shortest_repeat_spacing = sp;
    }
    uint32_t right_extension_length = 0;
    uint32_t max_right_extension_length = shortest_repeat_spacing - (uint32_t)minSpacerLength;
    int DR_index_end = (int)end_index;
    while (max_right_extension_length > 0) {
        if ((last_repeat_start_index + (uint32_t)searchWindowLength + right_extension_length) >= seqlen) DR_index_end -= 2;
        int cnt[4] = {0, 0, 0, 0};
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        for (int k = 0; k < DR_index_end; k += 2) {
            const uint32_t pos = ln_ss(h, k) + (uint32_t)h.replen;
            if (pos >= seqlen) break;
            const uint32_t b = ln_base(h, (int)pos);
            c0 += (b == 0); c1 += (b == 1); c2 += (b == 2); c3 += (b == 3);
        }
        (void)cnt;
        if ((c0 >= cut_off) || (c1 >= cut_off) || (c2 >= cut_off) || (c3 >= cut_off)) {
            h.replen++; max_right_extension_length--; right_extension_length++;
        } else break;
    }
    uint32_t left_extension_length = 0;
    const int test_for_negative = (int)(shortest_repeat_spacing - (uint32_t)h.replen);
    const uint32_t max_left_extension_length = (test_for_negative >= 0) ? (uint32_t)test_for_negative : 0;
    uint32_t DR_index_start = 0;
    while (left_extension_length < max_left_extension_length) {
        if ((int)first_repeat_start_index - (int)left_extension_length <= 0) DR_index_start += 2;
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        for (uint32_t k = DR_index_start; k < end_index; k += 2) {
            const int idx = (int)(ln_ss(h, (int)k) - left_extension_length - 1);
            if (idx < 0 || idx >= h.L) continue;
            const uint32_t b = ln_base(h, idx);
            c0 += (b == 0); c1 += (b == 1); c2 += (b == 2); c3 += (b == 3);
        }
        if ((c0 >= cut_off) || (c1 >= cut_off) || (c2 >= cut_off) || (c3 >= cut_off)) {
            h.replen++; left_extension_length++;
        } else break;
    }
    for (int r = 0; r + 1 < h.nss; r += 2) {
        uint32_t a = ln_ss(h, r), b = ln_ss(h, r + 1);
        a = (a < left_extension_length) ? 0 : a - left_extension_length;
        b = (b + right_extension_length >= seqlen) ? seqlen - 1 : b + right_extension_length;
        ln_ss_set(h, r, a); ln_ss_set(h, r + 1, b);
    }
    return (uint32_t)h.replen;
}

// Bit-parallel distance (see lane_lev_bp: Hyyro's OSA recurrences with the reference's transposition term restricted to
// i > 2 && j > 2, PatternMatcher.cpp:181-186) between read[s0, s0+n) and read[t0, t0+m), n <= m, n <= 8 * sizeof(WORD),
// m <= 64, both strings in registers.  stop_at >= 0: the caller only wants to know whether the distance is < stop_at —
// the bottom-row score changes by at most 1 per column, so once score - (columns left) >= stop_at the answer is "no" and
// stop_at is returned (any value >= stop_at would do).
template <typename WORD>
static __device__ __forceinline__ int ln_lev_regs(uint64_t s_lo, uint64_t s_hi, int n, uint64_t t_lo, uint64_t t_hi, int m, int stop_at)
{
    uint64_t q0, q1;
    ln_planes(s_lo, s_hi, n, q0, q1);
    const uint64_t nm = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    const WORD pm0 = (WORD)(~q0 & ~q1 & nm), pm1 = (WORD)(q0 & ~q1), pm2 = (WORD)(~q0 & q1 & nm), pm3 = (WORD)(q0 & q1);
    WORD VP = ~(WORD)0, VN = 0, D0 = 0, PMold = 0;
    int dist = n;
    const int topbit = n - 1;
    const WORD top = (WORD)1 << topbit;
    for (int j = 0; j < m; j++) {
        const uint32_t c = (uint32_t)((j < 32 ? t_lo >> (2 * j) : t_hi >> (2 * (j - 32))) & 3ull);
        const WORD PMj = (c & 2u) ? ((c & 1u) ? pm3 : pm2) : ((c & 1u) ? pm1 : pm0);         // three selects instead of four masked ors
        WORD TR = (WORD)((((WORD)~D0) & PMj) << 1) & PMold & ~(WORD)3;
        if (j < 2) TR = 0;
        D0 = (WORD)((WORD)((WORD)(PMj & VP) + VP) ^ VP) | PMj | VN;
        D0 |= TR;
        WORD HP = VN | (WORD)~(D0 | VP);
        WORD HN = D0 & VP;
        dist += (int)((HP & top) != 0) - (int)((HN & top) != 0);
        HP = (WORD)(HP << 1) | (WORD)1;
        HN = (WORD)(HN << 1);
        VP = HN | (WORD)~(D0 | HP);
        VN = HP & D0;
        PMold = PMj;
        if (stop_at >= 0 && dist - (m - 1 - j) >= stop_at) return stop_at;
    }
    return dist;
}

// bit-parallel distance between read[s0, s0+n) and read[t0, t0+m) on 2-bit codes, one base per LDS access (strings
// longer than 64 bases: only reachable with DR / spacer bounds far above the defaults)
template <typename WORD>
static __device__ __forceinline__ int ln_lev_core(const LaneRead &h, int s0, int n, int t0, int m)
{
    WORD pm0 = 0, pm1 = 0, pm2 = 0, pm3 = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t c = ln_base(h, s0 + i);
        const WORD b = (WORD)1 << i;
        pm0 |= b & ((WORD)0 - (WORD)(c == 0)); pm1 |= b & ((WORD)0 - (WORD)(c == 1));
        pm2 |= b & ((WORD)0 - (WORD)(c == 2)); pm3 |= b & ((WORD)0 - (WORD)(c == 3));
    }
    WORD VP = ~(WORD)0, VN = 0, D0 = 0, PMold = 0;
    int dist = n;
    const int topbit = n - 1;
    for (int j = 0; j < m; j++) {
        const uint32_t c = ln_base(h, t0 + j);
        const WORD PMj = (pm0 & ((WORD)0 - (WORD)(c == 0))) | (pm1 & ((WORD)0 - (WORD)(c == 1))) |
                         (pm2 & ((WORD)0 - (WORD)(c == 2))) | (pm3 & ((WORD)0 - (WORD)(c == 3)));
        WORD TR = (WORD)((((WORD)~D0) & PMj) << 1) & PMold & ~(WORD)3;
        TR &= (WORD)0 - (WORD)(j >= 2);
        D0 = (WORD)((WORD)((WORD)(PMj & VP) + VP) ^ VP) | PMj | VN;
        D0 |= TR;
        WORD HP = VN | (WORD)~(D0 | VP);
        WORD HN = D0 & VP;
        dist += (int)((HP >> topbit) & 1) - (int)((HN >> topbit) & 1);
        HP = (WORD)(HP << 1) | (WORD)1;
        HN = (WORD)(HN << 1);
        VP = HN | (WORD)~(D0 | HP);
        VN = HP & D0;
        PMold = PMj;
    }
    return dist;
}

// edit distance of read[s0, s0+n) and read[t0, t0+m); sets h.punt when the pair needs the wavefront DP.  stop_at: see
// ln_lev_regs (-1: the exact distance)
static __device__ int ln_distance(LaneRead &h, int s0, int n, int t0, int m, int stop_at)
{
    if (n > m) { int x = s0; s0 = t0; t0 = x; x = n; n = m; m = x; }
    if (n > 64) { h.punt = 1; return 0; }
    if (m <= 64) {
        uint64_t sl, sh, tl, th;
        ln_load128(h, s0, sl, sh); ln_load128(h, t0, tl, th);
        // (one instantiation for every pair: a wave whose pairs fall on both sides of 32 would issue both loops in turn)
        return ln_lev_regs<uint64_t>(sl, sh, n, tl, th, m, stop_at);
    }
    return (n <= 32) ? ln_lev_core<uint32_t>(h, s0, n, t0, m) : ln_lev_core<uint64_t>(h, s0, n, t0, m);
}

// qcFoundRepeats, libcrispr.cpp:869-1029, in the lane.  Its similarity tests — getStringSimilarity (PatternMatcher.cpp:197-204)
// as a value or as "(double)similarity > 0.82" — are ONE site in one loop (ln_distance's three loops exist once here, not once
// per test of the source): which pair comes next, and what becomes of the result, is chosen around it.
//   two repeats      one threshold test: repeat vs spacer
//   three repeats    two threshold tests: spacer vs spacer, repeat vs spacer.  ONE comparison, so every average is the single
//                    value itself (x / 1.0f == x) and the tests are plain threshold tests
//   four and more    per spacer but the last: repeat vs spacer and spacer vs next spacer as values, averaged
// A threshold test may stop early: the similarity falls monotonically with the distance, so the smallest distance d_no whose
// similarity is NOT above the cut is found first (with the reference's own float expression) and the DP stops as soon as the
// distance is known to reach it (ln_lev_regs).  A pair that needs the wavefront DP sets h.punt, and every path then returns 0.
static __device__ __forceinline__ int ln_qc(LaneRead &h, int minSpacerLength, int maxSpacerLength, uint32_t dbg)
{
    if (dbg == 6) return 1;                             // (CRASS_SURV_DEBUG, timing breakdown only)
    const int num_repeats = h.nss / 2;
    if (num_repeats < 2) return -1;
    uint32_t rep_len;
    const uint32_t rep_start = ln_ss(h, 0);
    if (!substr_len(h.L, rep_start, ln_ss(h, 1) - rep_start + 1, rep_len)) return -1;
    {   // isRepeatLowComplexity (:1031-1069); packed reads hold A/C/G/T only
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        if (rep_len <= 64) {                            // base counts from the two bit planes
            uint64_t lo, hi, p0, p1;
            ln_load128(h, (int)rep_start, lo, hi);
            ln_planes(lo, hi, (int)rep_len, p0, p1);
            c3 = __popcll(p0 & p1); c1 = __popcll(p0 & ~p1); c2 = __popcll(~p0 & p1); c0 = (int)rep_len - c1 - c2 - c3;
        } else
            for (uint32_t i = 0; i < rep_len; i++) { const uint32_t b = ln_base(h, (int)(rep_start + i)); c0 += (b == 0); c1 += (b == 1); c2 += (b == 2); c3 += (b == 3); }
        const int cut_off = (int)((double)(int)rep_len * 0.75);
        if (c0 > cut_off || c3 > cut_off || c2 > cut_off || c1 > cut_off) return 0;
    }
    if (dbg == 5) return 1;
    const int nsp = num_repeats - 1;
    const int mode = nsp < 2 ? 0 : (nsp == 2 ? 1 : 2);       // two repeats / three / four and more
    float ave_spacer_to_spacer_len_difference = 0.0f, ave_repeat_to_spacer_len_difference = 0.0f;
    float ave_spacer_to_spacer_difference = 0.0f, ave_repeat_to_spacer_difference = 0.0f;
    int min_spacer_length = 10000000, max_spacer_length = 0, num_compared = 0;
    uint32_t cur_start = ln_ss(h, 1) + 1, cur_len = 0, nxt_start = 0, nxt_len = 0;
    if (mode == 0) {
        const uint32_t e = ln_ss(h, 2) - 1;
        if (!substr_len(h.L, cur_start, e - cur_start, cur_len)) return -1;
        if ((int)cur_len < minSpacerLength) return 0;
        if ((int)cur_len > maxSpacerLength) return 0;
    } else {
        if (!substr_len(h.L, cur_start, ln_ss(h, 2) - cur_start, cur_len)) return -1;
        if (mode == 1) {
            nxt_start = ln_ss(h, 3) + 1;
            if (!substr_len(h.L, nxt_start, ln_ss(h, 4) - nxt_start, nxt_len)) return -1;
            const int mn = (int)(cur_len < nxt_len ? cur_len : nxt_len), mx = (int)(cur_len > nxt_len ? cur_len : nxt_len);
            if (mn < minSpacerLength || mx > maxSpacerLength) return 0;
        }
    }
    const int n_tests = mode == 0 ? 1 : (mode == 1 ? 2 : 2 * (nsp - 1));
    for (int k = 0; k < n_tests; k++) {
        bool rep_vs_cur;                                 // this test's pair: repeat vs current spacer, else current vs next spacer
        if (mode == 2) {
            rep_vs_cur = !(k & 1);
            if (rep_vs_cur) {                            // spacer k / 2 of the loop at :935-975
                if ((int)cur_len < min_spacer_length) min_spacer_length = (int)cur_len;
                if ((int)cur_len > max_spacer_length) max_spacer_length = (int)cur_len;
                nxt_start = ln_ss(h, k + 3) + 1;
                if (!substr_len(h.L, nxt_start, ln_ss(h, k + 4) - nxt_start, nxt_len)) return -1;
                num_compared++;
            }
        } else rep_vs_cur = mode == 0 || k == 1;
        const int s0 = rep_vs_cur ? (int)rep_start : (int)cur_start, n = rep_vs_cur ? (int)rep_len : (int)cur_len;
        const int t0 = rep_vs_cur ? (int)cur_start : (int)nxt_start, m = rep_vs_cur ? (int)cur_len : (int)nxt_len;
        float sim = 0.0f;                                // a string below three bases: similarity 0
        if (!(n < 3 || m < 3)) {
            const float max_length = (float)(n > m ? n : m);
            int stop_at = -1;
            if (mode != 2) {
                stop_at = 0;
                while (stop_at <= (n > m ? n : m) && (double)(float)(1.0 - (double)((float)stop_at / max_length)) > 0.82) stop_at++;
            }
            const int d = ln_distance(h, s0, n, t0, m, stop_at);
            if (h.punt) return 0;
            sim = (float)(1.0 - (double)((float)d / max_length));
        }
        if (mode != 2) {
            if ((double)sim > 0.82) return 0;
        } else if (rep_vs_cur) ave_repeat_to_spacer_difference += sim;
        else {
            float ss_diff = 0;
            ss_diff += sim;
            ave_spacer_to_spacer_difference += ss_diff;
            ave_spacer_to_spacer_len_difference += ((float)cur_len - (float)nxt_len);
            ave_repeat_to_spacer_len_difference += ((float)rep_len - (float)cur_len);
            cur_start = nxt_start; cur_len = nxt_len;
        }
    }
    if (mode == 0) {
        int dlen = (int)cur_len - (int)rep_len;
        if (dlen < 0) dlen = -dlen;
        if (dlen > 30) return 0;
        return 1;
    }
    if (mode == 1) {
        if ((int)fabsf(((float)cur_len - (float)nxt_len) / 1.0f) > 12) return 0;
        if ((int)fabsf(((float)rep_len - (float)cur_len) / 1.0f) > 30) return 0;
        return 1;
    }
    if ((int)cur_len < min_spacer_length) min_spacer_length = (int)cur_len;       // the last spacer
    if ((int)cur_len > max_spacer_length) max_spacer_length = (int)cur_len;
    ave_spacer_to_spacer_difference /= (float)num_compared;
    ave_repeat_to_spacer_difference /= (float)num_compared;
    ave_spacer_to_spacer_len_difference /= (float)num_compared;
    ave_spacer_to_spacer_len_difference = fabsf(ave_spacer_to_spacer_len_difference);
    ave_repeat_to_spacer_len_difference /= (float)num_compared;
    ave_repeat_to_spacer_len_difference = fabsf(ave_repeat_to_spacer_len_difference);
    if (min_spacer_length < minSpacerLength) return 0;
    if (max_spacer_length > maxSpacerLength) return 0;
    if ((double)ave_spacer_to_spacer_difference > 0.82) return 0;
    if ((double)ave_repeat_to_spacer_difference > 0.82) return 0;
    if ((int)ave_spacer_to_spacer_len_difference > 12) return 0;
    if ((int)ave_repeat_to_spacer_len_difference > 30) return 0;
    return 1;
}

// ---- the QC's threshold tests as TASKS of the block (k_survivor_lanes) ----
// qcFoundRepeats spends its time in one or two "similarity > 0.82" tests per candidate (two repeats: repeat vs spacer; three:
// spacer vs spacer, repeat vs spacer) — bit-parallel edit distances of ~40 columns.  Run by the candidate's own lane they
// occupied the third of a block's lanes that hold real CRISPR reads, once or twice in a row, while the other lanes of the block
// — reads that a chance seed hit let through — had long finished: 180 of the lane kernel's 520 us at 100 M reads.  The tests are
// therefore QUEUED in LDS by the candidates' lanes and run by ALL lanes of the block, a test per lane (any lane reads any
// lane's words: the rows are LDS), tests whose shorter string has at most 32 bases on 32-bit words from the queue's front, the
// others on 64-bit words from its back.  The decisions stay with the candidate's lane, in the reference's order.
struct QcTask { uint32_t a, b; };                 // a: owner thread (8) | s0 (9) | n (7) | d_no (7);  b: t0 (9) | m (7)
struct QcPool {
    QcTask *task;                                 // [2 * threads of the block]: 32-bit tests from the front, 64-bit ones from the back
    uint8_t *res;                                 // [2 * threads]: by task slot, 1 = "similarity above the cut"
    uint32_t *cnt;                                // [0] 32-bit tests queued, [1] 64-bit tests queued
    const uint32_t *rows;                         // the block's LDS rows (sl_lds)
    uint32_t wave_words;                          // words per wave's part of it
    uint32_t cap;                                 // 2 * threads
};
// what a lane remembers between queueing its tests and reading their results
struct QcPending { int kind; uint32_t slot_a, slot_b; uint32_t cur_len, nxt_len, rep_len, sp_len; };

// "(double)getStringSimilarity(a, b) > 0.82" as a queued test; returns the task's slot, or 0xFFFFFFFF with *now = the answer when
// it needs no distance (a string below three bases: similarity 0)
static __device__ uint32_t qc_enqueue_above(const QcPool &q, int s0, int n, int t0, int m, bool *now)
{
    *now = false;
    if (n < 3 || m < 3) { *now = 0.0 > 0.82; return 0xFFFFFFFFu; }
    if (n > m) { int x = s0; s0 = t0; t0 = x; x = n; n = m; m = x; }
    const float max_length = (float)m;
    int d_no = 0;
    while (d_no <= m && (double)(float)(1.0 - (double)((float)d_no / max_length)) > 0.82) d_no++;
    uint32_t slot;
    if (n <= 32) slot = atomicAdd(&q.cnt[0], 1u);
    else slot = q.cap - 1u - atomicAdd(&q.cnt[1], 1u);
    QcTask t;
    t.a = (uint32_t)threadIdx.x | ((uint32_t)s0 << 8) | ((uint32_t)n << 17) | ((uint32_t)d_no << 24);
    t.b = (uint32_t)t0 | ((uint32_t)m << 9);
    q.task[slot] = t;
    return slot;
}

// one queued test, by whichever lane drew it
template <typename WORD>
static __device__ __forceinline__ void qc_run_task(const QcPool &q, uint32_t slot)
{
    const QcTask t = q.task[slot];
    const uint32_t owner = t.a & 0xFFu;
    const int s0 = (int)((t.a >> 8) & 0x1FFu), n = (int)((t.a >> 17) & 0x7Fu), d_no = (int)(t.a >> 24);
    const int t0 = (int)(t.b & 0x1FFu), m = (int)(t.b >> 9);
    LaneRead ho;
    ho.w = q.rows + (size_t)(owner >> 6) * q.wave_words + (owner & 63u);
    uint64_t sl, sh, tl, th;
    ln_load128(ho, s0, sl, sh); ln_load128(ho, t0, tl, th);
    const int d = ln_lev_regs<WORD>(sl, sh, n, tl, th, m, d_no);
    q.res[slot] = (double)(float)(1.0 - (double)((float)d / (float)m)) > 0.82 ? 1 : 0;
}

// qcFoundRepeats (libcrispr.cpp:869-1029) up to its similarity tests: -1 / 0 / 1 = decided here (ln_qc's values); 2 = the
// candidate's tests are queued (pd says which), qc_pool_end decides; 3 = candidates of four repeats or more, and strings beyond
// 64 bases: ln_qc as before (rare at these read lengths), from qc_pool_begin's ONE call of it.
static __device__ __forceinline__ int qc_pool_begin_queued(LaneRead &h, int minSpacerLength, int maxSpacerLength, uint32_t dbg, const QcPool &q, QcPending &pd)
{
    pd.kind = 0;
    const int num_repeats = h.nss / 2;
    if (dbg == 5 || dbg == 6 || num_repeats < 2 || num_repeats > 3) return 3;
    uint32_t rep_len;
    const uint32_t rep_start = ln_ss(h, 0);
    if (!substr_len(h.L, rep_start, ln_ss(h, 1) - rep_start + 1, rep_len)) return -1;
    if (rep_len > 64) return 3;
    {   // isRepeatLowComplexity (:1031-1069); packed reads hold A/C/G/T only
        uint64_t lo, hi, p0, p1;
        ln_load128(h, (int)rep_start, lo, hi);
        ln_planes(lo, hi, (int)rep_len, p0, p1);
        const int c3 = __popcll(p0 & p1), c1 = __popcll(p0 & ~p1), c2 = __popcll(~p0 & p1), c0 = (int)rep_len - c1 - c2 - c3;
        const int cut_off = (int)((double)(int)rep_len * 0.75);
        if (c0 > cut_off || c3 > cut_off || c2 > cut_off || c1 > cut_off) return 0;
    }
    if (num_repeats == 3) {
        uint32_t cur_start = ln_ss(h, 1) + 1, cur_len;
        if (!substr_len(h.L, cur_start, ln_ss(h, 2) - cur_start, cur_len)) return -1;
        uint32_t nxt_start = ln_ss(h, 3) + 1, nxt_len;
        if (!substr_len(h.L, nxt_start, ln_ss(h, 4) - nxt_start, nxt_len)) return -1;
        const int mn = (int)(cur_len < nxt_len ? cur_len : nxt_len), mx = (int)(cur_len > nxt_len ? cur_len : nxt_len);
        if (mn < minSpacerLength || mx > maxSpacerLength) return 0;
        if (cur_len > 64 || nxt_len > 64) return 3;
        bool a_now, b_now;
        pd.slot_a = qc_enqueue_above(q, (int)cur_start, (int)cur_len, (int)nxt_start, (int)nxt_len, &a_now);
        if (pd.slot_a == 0xFFFFFFFFu && a_now) return 0;
        pd.slot_b = qc_enqueue_above(q, (int)rep_start, (int)rep_len, (int)cur_start, (int)cur_len, &b_now);
        if (pd.slot_b == 0xFFFFFFFFu && b_now) return 0;          // (its own test only: a queued first test is not waited for — both "return 0")
        pd.kind = 3; pd.cur_len = cur_len; pd.nxt_len = nxt_len; pd.rep_len = rep_len;
        return 2;
    }
    // two repeats
    uint32_t s = ln_ss(h, 1) + 1;
    uint32_t e = ln_ss(h, 2) - 1;
    uint32_t sp_len;
    if (!substr_len(h.L, s, e - s, sp_len)) return -1;
    if ((int)sp_len < minSpacerLength) return 0;
    if ((int)sp_len > maxSpacerLength) return 0;
    if (sp_len > 64) return 3;
    bool now;
    pd.slot_a = qc_enqueue_above(q, (int)rep_start, (int)rep_len, (int)s, (int)sp_len, &now);
    if (pd.slot_a == 0xFFFFFFFFu && now) return 0;
    pd.slot_b = 0xFFFFFFFFu;
    pd.kind = 2; pd.sp_len = sp_len; pd.rep_len = rep_len;
    return 2;
}
static __device__ __forceinline__ int qc_pool_begin(LaneRead &h, int minSpacerLength, int maxSpacerLength, uint32_t dbg, const QcPool &q, QcPending &pd)
{
    const int r = qc_pool_begin_queued(h, minSpacerLength, maxSpacerLength, dbg, q, pd);
    if (__builtin_expect(r == 3, 0)) return ln_qc(h, minSpacerLength, maxSpacerLength, dbg);
    return r;
}
// ... and from the tests' results on (same values as ln_qc)
static __device__ int qc_pool_end(const QcPool &q, const QcPending &pd)
{
    const bool a = pd.slot_a != 0xFFFFFFFFu && q.res[pd.slot_a] != 0;
    if (pd.kind == 3) {
        if (a) return 0;
        const bool b = pd.slot_b != 0xFFFFFFFFu && q.res[pd.slot_b] != 0;
        if (b) return 0;
        if ((int)fabsf(((float)pd.cur_len - (float)pd.nxt_len) / 1.0f) > 12) return 0;
        if ((int)fabsf(((float)pd.rep_len - (float)pd.cur_len) / 1.0f) > 30) return 0;
        return 1;
    }
    if (a) return 0;
    int dlen = (int)pd.sp_len - (int)pd.rep_len;
    if (dlen < 0) dlen = -dlen;
    if (dlen > 30) return 0;
    return 1;
}

// active: this thread holds a read (the others only take part in the block's barriers and run queued tests)
static __device__ int ln_search_core(LaneRead &h, const DevParams &o, uint64_t seed_hint, bool active, const QcPool &pool)
{   // searchCore, libcrispr.cpp:265-395
    const uint32_t seq_length = (uint32_t)h.L;
    const uint32_t skips = o.skips;
    int searchEnd = (int)(seq_length - o.lowDR - o.lowSp - o.window - 1);
    h.nss = 0;
    bool on_lattice = true;
    uint32_t lattice_i = 0;
    uint32_t j = 0;
    // Two nested loops instead of the reference's one: the inner loop advances a lane from seed to seed (find, chain,
    // extend — cheap since the closed-form extension) until it holds a candidate that is due for qcFoundRepeats or has
    // run out of seeds; only then do the lanes of the wave that hold such a candidate run the QC, together.  The
    // sequence of events per read is the reference's; what changes is that the QC code — by far the longest stretch —
    // is issued once per round for the whole wave instead of once per seed iteration in which some lane needs it
    // (lanes reach their first QC in different iterations: 51 us of the kernel's 117 were QC issue slots).
    bool finished = !active || searchEnd < 0; int result = 0;      // this lane's searchCore has returned `result`
    for (;;) {
        bool ready = false, error = false, out_of_seeds = false;
        // (wave-uniform loop condition: the lanes leave this loop TOGETHER, whatever the compiler makes of the control flow)
        while (__any((int)(!finished && !ready && !out_of_seeds && !error))) {
            if (finished || ready || out_of_seeds || error) continue;
            // Each lane first walks (cheaply) to ITS next seed worth evaluating.  A lattice seed whose hint bit is
            // clear is a no-op iteration in the reference (no hit => no start/stops => numRepeats 0): skipping it
            // changes nothing.
            while (on_lattice && j <= (uint32_t)searchEnd && lattice_i < 64 && !((seed_hint >> lattice_i) & 1ull)) { j += skips; lattice_i++; }
            if (j > (uint32_t)searchEnd) { out_of_seeds = true; continue; }
            if (on_lattice) lattice_i++;
            uint32_t beginSearch = j + o.lowDR + o.lowSp;
            uint32_t endSearch = j + o.highDR + o.highSp + o.window;
            if (endSearch >= seq_length) endSearch = seq_length - 1;
            if (endSearch < beginSearch) endSearch = beginSearch;
            if (beginSearch > seq_length) { error = true; continue; }
            int pos = ln_find(h, (int)beginSearch, (int)endSearch, (int)j, (int)o.window, o.find_serial);
            if (o.debug_stop == 2) pos = -1;                // (CRASS_SURV_DEBUG, timing breakdown only: seed finds alone)
            if (pos >= 0) {
                ln_add(h, j, j + o.window - 1);
                ln_add(h, (uint32_t)pos, (uint32_t)pos + o.window - 1);
                if (!h.punt) ln_scan_right(h, (int)j, o.window, o.lowSp, 24, o.find_serial);
                if (h.punt) { finished = true; result = 0; continue; }
            }
            if ((uint32_t)(h.nss / 2) >= o.minRepeats) {
                uint32_t actual_repeat_length = ln_extend(h, (int)o.window, (int)o.lowSp);
                if (o.debug_stop != 3 && (actual_repeat_length >= o.lowDR) && (actual_repeat_length <= o.highDR)) { ready = true; continue; }    // (3: no QC)
                j = ln_ss(h, h.nss - 1) - 1;
                on_lattice = false;
            }
            h.nss = 0;
            j = j + skips;
        }
        if (!finished && error) { finished = true; result = -1; }
        if (!finished && out_of_seeds) { finished = true; result = 0; }
        // From here on the BLOCK moves together (three barriers per round, one or two rounds): the lanes that hold a candidate
        // queue its similarity tests, every lane of the block runs queued tests, the candidates' lanes decide.
        if (!__syncthreads_or((int)(!finished))) break;
        QcPending pd;
        pd.kind = 0;
        int qc = 0;
        if (!finished) qc = qc_pool_begin(h, (int)o.lowSp, (int)o.highSp, o.debug_stop, pool, pd);
        __syncthreads();
        {
            const uint32_t n32 = pool.cnt[0], n64 = pool.cnt[1];
            for (uint32_t t = threadIdx.x; t < n32; t += blockDim.x) qc_run_task<uint32_t>(pool, t);
            // (the 64-bit tests from the block's last lanes downwards: the waves that took 32-bit tests take these last)
            for (uint32_t t = blockDim.x - 1u - threadIdx.x; t < n64; t += blockDim.x) qc_run_task<uint64_t>(pool, pool.cap - 1u - t);
        }
        __syncthreads();
        if (threadIdx.x == 0) { pool.cnt[0] = 0u; pool.cnt[1] = 0u; }      // (the next round queues behind this round's first barrier)
        if (!finished) {
            if (qc == 2) qc = qc_pool_end(pool, pd);
            if (h.punt) { finished = true; result = 0; }
            else if (qc < 0) { finished = true; result = -1; }
            else if (qc) { finished = true; result = 1; }
            else {
                j = ln_ss(h, h.nss - 1) - 1;                // a rejected candidate: on with the seeds behind it (:390)
                on_lattice = false;
                h.nss = 0;
                j = j + skips;
            }
        }
    }
    return result;
}

// SL_WAVES waves per block.  A third of the survivors are real CRISPR reads (scan, extension, QC, orientation: the whole
// searchCore), the rest are spurious seed hits that leave after one window — and in slot order every wave holds ~21 of the former,
// so every wave runs for as long as its slowest lane with a third of its lanes busy.  The block therefore deals its 64 x SL_WAVES
// slots out by expected work: reads with at least two hinted lattice seeds (a repeat with a copy one unit on gives several; a
// chance match gives one) first, in slot order, then the others.  Each lane still writes its own slot: the result arrays do not
// notice.  PMC at 100 M reads: 318 M -> 224 M VALU wave instructions (8-wave blocks); 4 waves per block is the measured optimum
// (590 us in slot order with one wave per block -> 550; 8 waves 593, 16 waves 754: a block holds its LDS until its slowest wave ends).
#define SL_WAVES 4
// hint bit i of a lane's read = "lattice seed i may have a copy in its window", for the first 64 seeds; the others are walked.
// From the lane-per-read filter's word (32 seeds: reads of up to 256 bases) or from the read's position hints (bit 8 i of the
// bitmap: k_hint_positions filled the lattice class and cleared what lies behind searchEnd) — bit 0 of each byte, gathered by one
// multiplication per 64 positions (the partial products 2^(56 + 8k - 7j) of bits 8k and multiplier terms 2^(56 - 7j) are all
// distinct, and only those with k == j fall into the top byte)
static __device__ __forceinline__ uint64_t ln_hint64(const DevReads &R, const uint32_t *seed_hint, uint64_t r, int L, uint32_t skips)
{
    if (seed_hint) return 0xFFFFFFFF00000000ull | (uint64_t)seed_hint[r];
    if (!R.pos_hint) return ~0ull;
    const uint64_t *ph = R.pos_hint + rd_hint_off(R, r);
    const int nh = (L + 63) >> 6;
    if (R.hint_all) {
        // every position has a bit (another window or seed lattice): seed i sits at i * skips
        uint64_t hint = 0;
        for (uint32_t i = 0, p = 0; i < 64u && (int)p < L; i++, p += skips) hint |= ((ph[p >> 6] >> (p & 63u)) & 1ull) << i;
        return hint;
    }
    uint64_t hint = 0;
    for (int k = 0; k < 8 && k < nh; k++)
        hint |= (((ph[k] & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56) << (8 * k);
    return hint;
}
__global__ __launch_bounds__(WAVE * SL_WAVES) void k_survivor_lanes(DevReads R, DevParams P, const uint64_t *surv_idx, const uint32_t *d_n_surv,
                                                         uint64_t n_max, SurvOut *out, char *dr_chars, uint32_t dr_stride,
                                                         uint32_t *ss_pool, uint32_t ss_cap, uint8_t *found_flag,
                                                         const uint32_t *seed_hint, uint32_t words_per_read, DevMerge IM, int do_init, int regroup,
                                                         uint32_t *punt_cnt)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sl_lds[];
    __shared__ uint16_t sl_perm[WAVE * SL_WAVES];
    __shared__ uint32_t sl_cnt[SL_WAVES];
    __shared__ uint32_t sl_hint[WAVE * SL_WAVES];       // the slots' filter hints, read once (for the regrouping) and handed to whoever gets the slot
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
    // the tables of the merge that follows this stage are cleared on the way (stores next to an issue-bound kernel)
    if (do_init) dm_init_slice(IM, blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
    uint64_t n_surv = *d_n_surv;
    if (n_surv > n_max) n_surv = n_max;
    uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (regroup) {
        bool heavy = false;
        if (s < n_surv) {
            const uint64_t r0 = surv_idx[s];
            const uint32_t h0 = seed_hint ? seed_hint[r0] : 0u;
            sl_hint[threadIdx.x] = h0;
            heavy = !rd_is_exc(R, r0) && (seed_hint ? __popc(h0) : __popcll(ln_hint64(R, nullptr, r0, (int)rd_len(R, r0), P.skips))) >= 2;
        }
        const uint64_t hb = __ballot(heavy);
        if (lane == 0) sl_cnt[wv] = (uint32_t)__popcll(hb);
        __syncthreads();
        uint32_t heavy_before = 0, heavy_total = 0;
#pragma unroll
        for (int k = 0; k < SL_WAVES; k++) { const uint32_t c = sl_cnt[k]; heavy_total += c; if (k < wv) heavy_before += c; }
        const uint32_t below = (uint32_t)__popcll(hb & ((1ull << lane) - 1ull));
        const uint32_t pos = heavy ? heavy_before + below
                                   : heavy_total + ((uint32_t)wv * WAVE - heavy_before) + ((uint32_t)lane - below);
        // (rotating which wave of the block gets the heavy slots, so that one SIMD of a CU does not run every block's long wave:
        // measured, no difference — 114 vs 113 us for an eighth of the 100 M reads, 4.19 vs 4.13 ms at 100 M; NOTES r06)
        sl_perm[pos] = (uint16_t)threadIdx.x;
        __syncthreads();
        s = blockIdx.x * (uint64_t)blockDim.x + sl_perm[threadIdx.x];
    }
    const bool hint_in_lds = regroup && seed_hint;
    const size_t wave_words = (size_t)(words_per_read + 5) * WAVE + ((size_t)ss_cap * WAVE + 1) / 2;      // this wave's part of the LDS
    uint32_t *wbase = sl_lds + (size_t)wv * wave_words;
    uint32_t *lw = wbase + lane;                                       // [word][lane]
    uint16_t *lss = reinterpret_cast<uint16_t *>(wbase + (size_t)(words_per_read + 5) * WAVE) + lane;   // [entry][lane]
    // (no thread leaves before the end: the block's lanes run the candidates' queued similarity tests together, QcPool)
    static_assert(WAVE * SL_WAVES <= 256, "QcTask keeps the owner's thread index in 8 bits");
    __shared__ QcTask sl_task[2 * WAVE * SL_WAVES];
    __shared__ uint8_t sl_res[2 * WAVE * SL_WAVES];
    __shared__ uint32_t sl_qcnt[2];
    if (threadIdx.x < 2) sl_qcnt[threadIdx.x] = 0u;      // (the first queueing is behind ln_search_core's first barrier)
    QcPool pool;
    pool.task = sl_task; pool.res = sl_res; pool.cnt = sl_qcnt; pool.rows = sl_lds; pool.wave_words = (uint32_t)wave_words; pool.cap = 2 * WAVE * SL_WAVES;
    bool active = s < n_surv;
    const uint64_t r = active ? surv_idx[s] : 0;
    if (active && rd_is_exc(R, r)) {                    // raw-byte read: the wave kernel's exception pass (err == 5)
        SurvOut o;
        o.found = 0; o.n_ss = 0; o.repeat_len = 0; o.ss_off = 0; o.dr_len = 0; o.low_lexi = 0; o.err = 5;
        out[s] = o;
        active = false;
    }
    const int L = active ? (int)rd_len(R, r) : 0;
    const uint32_t *g = R.packed + (active ? rd_word_off(R, r) : 0);
    const int nw = (L + 15) >> 4;
    // (a row is dword-aligned only, which global_load_dwordx4 takes on gfx950 — ff_load_row: three or four wide loads per lane
    // instead of ten to sixteen single words, every one of which was 64 lines' worth of look-ups for the wave)
    {
        int i = 0;
        for (; i + 4 <= nw; i += 4) {
            const ff_u32x4 v = *reinterpret_cast<const ff_u32x4 *>(g + i);
            lw[i * WAVE] = v.x; lw[(i + 1) * WAVE] = v.y; lw[(i + 2) * WAVE] = v.z; lw[(i + 3) * WAVE] = v.w;
        }
        for (; i < nw; i++) lw[i * WAVE] = g[i];
        for (; i < (int)words_per_read + 5; i++) lw[i * WAVE] = 0u;                             // (ln_load128 reads up to 4 words past a base)
    }
    LaneRead h;
    h.w = lw; h.ss = lss; h.L = L; h.nss = 0; h.cap = (int)ss_cap; h.replen = 0; h.punt = 0;
    h.cmask = (1u << (2 * P.window)) - 1u;
    const uint64_t hint = !active ? 0ull : hint_in_lds ? (0xFFFFFFFF00000000ull | (uint64_t)sl_hint[(uint32_t)(s - blockIdx.x * (uint64_t)blockDim.x)]) : ln_hint64(R, seed_hint, r, L, P.skips);
    int f = (P.debug_stop == 1) ? 0 : ln_search_core(h, P, hint, active, pool);      // (1: load only)
    if (!active) return;
    if (P.debug_stop == 4 && f == 1) f = 0;                           // (4: no orientation / output)
    SurvOut o;
    o.found = 0; o.n_ss = 0; o.repeat_len = 0; o.ss_off = 0; o.dr_len = 0; o.low_lexi = 0; o.err = 0;
    if (h.punt) { o.err = 4; if (punt_cnt) atomicAdd(punt_cnt, 1u); }      // (counted: the wave kernel's launch behind this one leaves at once when there is none)
    else if (f < 0) o.err = 1;
    else if (f == 1) {
        // ReadHolder::DRLowLexi (ReadHolder.cpp:513-591): representative repeat, orientation
        const int num_repeats = h.nss / 2;
        int pick;
        if (num_repeats == 1) pick = 0;
        else if (num_repeats == 2) {
            if (ln_ss(h, 0) == 0) pick = 2;
            else if (ln_ss(h, h.nss - 1) == (uint32_t)L) pick = 0;
            else pick = ((int)(ln_ss(h, 1) - ln_ss(h, 0)) > (int)(ln_ss(h, 3) - ln_ss(h, 2))) ? 0 : 2;
        } else pick = 2;
        uint32_t dlen = 0;
        const uint32_t st = ln_ss(h, pick);
        if (!substr_len(L, st, ln_ss(h, pick + 1) - st + 1, dlen) || dlen > dr_stride) o.err = 1;
        else {
            int less = 0;
            char *dr = dr_chars + s * (uint64_t)dr_stride;
            const uint32_t off = (uint32_t)s * ss_cap;
            if (dlen <= 64 && (dr_stride & 15u) == 0) {
                // the repeat as a 128-bit value, its reverse complement by bit reversal, DRLowLexi's string comparison as
                // "first differing base from the low end" (as k_recruit_finish), the ASCII string four bases per word
                uint64_t v0, v1;
                ln_load128(h, (int)st, v0, v1);
                const uint64_t m0 = dlen >= 32 ? ~0ull : ((1ull << (2 * dlen)) - 1ull);
                const uint64_t m1 = dlen >= 64 ? ~0ull : (dlen > 32 ? ((1ull << (2 * (dlen - 32))) - 1ull) : 0ull);
                v0 &= m0; v1 &= m1;
                auto rev2 = [](uint64_t t) -> uint64_t { t = __brevll(t); return ((t >> 1) & 0x5555555555555555ull) | ((t & 0x5555555555555555ull) << 1); };
                const uint64_t c0 = rev2(~v1), c1 = rev2(~v0);
                const uint32_t drop = 128u - 2u * dlen;
                uint64_t r0, r1;
                if (drop == 0) { r0 = c0; r1 = c1; }
                else if (drop < 64) { r0 = (c0 >> drop) | (c1 << (64 - drop)); r1 = c1 >> drop; }
                else { r0 = c1 >> (drop - 64); r1 = 0; }
                r0 &= m0; r1 &= m1;
                const uint64_t d0 = v0 ^ r0, d1 = v1 ^ r1;
                if (d0 | d1) {
                    const uint64_t dv = d0 ? d0 : d1, av = d0 ? v0 : v1, bv = d0 ? r0 : r1;
                    const int p = (__ffsll((unsigned long long)dv) - 1) & ~1;
                    less = ((av >> p) & 3ull) < ((bv >> p) & 3ull);
                }
                const uint64_t s0 = less ? v0 : r0, s1 = less ? v1 : r1;
                uint4 *d4 = reinterpret_cast<uint4 *>(dr);
                for (uint32_t q = 0; q < dr_stride / 16; q++) {             // 16 bases = 32 bits of the packed string per uint4
                    const uint32_t bits = q < 2 ? (uint32_t)(s0 >> (32 * q)) : (q < 4 ? (uint32_t)(s1 >> (32 * (q - 2))) : 0u);
                    uint32_t wv[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t b8 = (bits >> (8 * k)) & 0xFFu;
                        const uint32_t Ls = ((b8 & 0x55u) * 0x00041041u) & 0x01010101u, Hs = (((b8 >> 1) & 0x55u) * 0x00041041u) & 0x01010101u;
                        uint32_t asc = 0x41414141u + (Ls << 1) + Hs * 6u + (Ls & Hs) * 0x0Bu;       // A 41, C 43, G 47, T 54
                        const int rem = (int)dlen - (int)(q * 16 + k * 4);                           // bases left from this word on
                        if (rem <= 0) asc = 0u; else if (rem < 4) asc &= (1u << (8 * rem)) - 1u;
                        wv[k] = asc;
                    }
                    uint4 o4; o4.x = wv[0]; o4.y = wv[1]; o4.z = wv[2]; o4.w = wv[3];
                    d4[q] = o4;
                }
                if (less) for (int k = 0; k < h.nss; k++) ss_pool[off + k] = ln_ss(h, k);
                else for (int k = 0; k < h.nss; k++) ss_pool[off + k] = (uint32_t)L - 1 - ln_ss(h, h.nss - 1 - k);   // reverseStartStops
            } else {
            for (uint32_t i = 0; i < dlen; i++) {
                const uint32_t a = ln_base(h, (int)(st + i)), b = 3u - ln_base(h, (int)(st + dlen - 1 - i));
                if (a != b) { less = a < b; break; }
            }
            if (less) {
                for (uint32_t i = 0; i < dr_stride; i++) dr[i] = (i < dlen) ? "ACGT"[ln_base(h, (int)(st + i))] : (char)0;
                for (int k = 0; k < h.nss; k++) ss_pool[off + k] = ln_ss(h, k);
            } else {
                for (uint32_t i = 0; i < dr_stride; i++) dr[i] = (i < dlen) ? "ACGT"[3u - ln_base(h, (int)(st + dlen - 1 - i))] : (char)0;
                for (int k = 0; k < h.nss; k++) ss_pool[off + k] = (uint32_t)L - 1 - ln_ss(h, h.nss - 1 - k);   // reverseStartStops
            }
            }
            o.found = 1; o.n_ss = (uint32_t)h.nss; o.repeat_len = (uint32_t)h.replen; o.ss_off = off;
            o.dr_len = (uint16_t)dlen; o.low_lexi = (uint8_t)less;
            found_flag[rd_header_id(R, r)] = 1;
        }
    }
    out[s] = o;
}

hipError_t launch_survivor_lanes(const DevReads &R, const DevParams &P, const uint64_t *surv_idx, const uint32_t *d_n_surv,
                                 uint64_t n_surv_max, SurvOut *out, char *dr_chars, uint32_t dr_stride, uint32_t *ss_pool,
                                 uint32_t ss_cap, uint8_t *found_flag, const uint32_t *seed_hint, hipStream_t st, const DevMerge *init_merge,
                                 uint32_t max_len, uint32_t *punt_cnt)
{
    if (n_surv_max == 0) return init_merge ? hipErrorNotSupported : hipSuccess;
    // a lane holds its read's words in LDS: reads of up to 512 bases (one stride or not: the rows are addressed per read)
    const uint32_t wpr = R.stride_words ? R.stride_words : (max_len + 15) / 16;
    if (!wpr || wpr > 32 || ss_cap > 64) return hipErrorNotSupported;
    const size_t wave_words = (size_t)(wpr + 5) * WAVE + ((size_t)ss_cap * WAVE + 1) / 2;
    const size_t lds = wave_words * 4 * SL_WAVES;
    static const bool no_regroup = getenv("CRASS_SURV_NO_REGROUP") != nullptr;      // A/B switch: lanes in slot order
    const unsigned bt = WAVE * SL_WAVES;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_survivor_lanes), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    CRASS_LAUNCH(k_survivor_lanes, dim3((unsigned)((n_surv_max + bt - 1) / bt)), dim3(bt), lds, st, R, P, surv_idx, d_n_surv,
                       n_surv_max, out, dr_chars, dr_stride, ss_pool, ss_cap, found_flag, seed_hint, wpr, init_merge ? *init_merge : DevMerge{},
                       init_merge ? 1 : 0, ((seed_hint || R.pos_hint) && !no_regroup) ? 1 : 0, punt_cnt);
    return hipGetLastError();
}

SurvLds survivor_lds_layout(uint32_t max_len, const DevParams &P, uint32_t row_len_cap, uint32_t seq_window_bytes, uint32_t ss_entries_cap)
{
    SurvLds l;
    l.seq_bytes = ((max_len + 16 + 16) + 15u) & ~15u;
    l.seq_window = 0;
    if (seq_window_bytes && ((seq_window_bytes + 15u) & ~15u) + 32u < l.seq_bytes) { l.seq_bytes = ((seq_window_bytes + 15u) & ~15u) + 32u; l.seq_window = l.seq_bytes - 32u; }
    uint32_t reps = max_len / (P.window + P.lowSp) + 4;
    l.ss_cap = ((2 * reps) + 3u) & ~3u;
    l.ss_slot = l.ss_cap;
    if (ss_entries_cap && ((ss_entries_cap + 3u) & ~3u) < l.ss_cap) l.ss_cap = (ss_entries_cap + 3u) & ~3u;
    l.row_elems = ((std::min(max_len, row_len_cap) + 8) + 7u) & ~7u;
    l.words_cap = (((max_len + 15) / 16 + 2) + 3u) & ~3u;
    l.hint_words = (((max_len + 63) / 64 + 2 + 1u) & ~1u) + 4u;      // + 8 x uint32: where each residue class's hint bits start (search_core)
    l.total_bytes = l.seq_bytes + l.ss_cap * 4 + 2 * l.row_elems * 2 + l.words_cap * 4 + l.ss_cap * 4 + l.hint_words * 8;
    return l;
}

// The layout of the last-resort launch: whole-read ASCII copy, full start/stop list, packed words, hint words, and rows.
// Rows sized by the set's longest read (max_len + 8 entries) pass a CU's 160 KB from ~28 000 bases on under the
// defaults (5.85 bytes per base) and on their own from 40 953.  They never need the read's length.  rowA / rowB are used by
// wave_similarity / wave_lev alone (row index <= the longer string's length), and those are reached
//   - in search_core only behind `actual_repeat_length <= highDR`; qc_found_repeats' rep_len is ss[1] - ss[0] + 1 of the
//     extended, clamped list, i.e. <= that length;
//   - with three repeats and more, only behind `max_spacer_length <= maxSpacerLength` (the length tests stand in front of every
//     edit distance), and the strings of the fallback loop are rep_len and two of those spacers;
//   - with two repeats, only behind `sp_len <= maxSpacerLength`.
// So `max(al, bl, rep_len) + 8 > row_cap` can only ever be asked for strings of at most max(highDR, highSp) bases, and rows of
// that + 8 entries hold every string the kernel compares: 1.85 bytes per base under the defaults (111 KB at 60 000 bases).
// A set that fits with rows of its longest read keeps that layout, byte for byte; the bound applies only where it does not.
// The caller refuses what still exceeds 160 KB (L + 32 + 8 ss_cap + 4 rows + L/4 + L/8 bytes, ss_cap = 2 (L / (w + lowSp) + 4)).
SurvLds survivor_lds_last_resort(uint32_t max_len, const DevParams &P)
{
    const SurvLds l = survivor_lds_layout(max_len, P);
    if (l.total_bytes <= 160 * 1024) return l;
    return survivor_lds_layout(max_len, P, std::max(P.highDR, P.highSp));
}

hipError_t launch_survivor(const DevReads &R, const DevParams &P, bool exceptions, const uint64_t *surv_idx,
                           const uint32_t *d_n_surv, uint64_t n_surv_max, SurvOut *out, char *dr_chars,
                           uint32_t dr_stride, uint32_t *ss_pool, uint32_t ss_pool_cap, uint32_t *d_ss_used,
                           uint8_t *found_flag, const uint32_t *seed_hint, const SurvLds &lds, int grid, hipStream_t st,
                           int punt_only, uint64_t slot_base, uint64_t slot_total, const uint32_t *punt_list, const uint32_t *d_punt_n, uint32_t *redo_list)
{
    if (n_surv_max == 0) return hipSuccess;
    hipError_t e;
    const uint32_t lds_bytes = ((lds.total_bytes + 7u) & ~7u) + (P.prof ? PF_LDS_WORDS * 8u : 0u);      // (diagnostics: the phase slots)
    if (exceptions) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_survivor<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        CRASS_LAUNCH(k_survivor<true>, dim3(grid), dim3(WAVE), lds_bytes, st, R, P, surv_idx, d_n_surv, n_surv_max,
                           out, dr_chars, dr_stride, ss_pool, ss_pool_cap, d_ss_used, found_flag, seed_hint, lds, punt_only, slot_base, slot_total, punt_list, d_punt_n, redo_list);
    } else {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_survivor<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        static const bool occ_dbg = getenv("CRASS_OCC_DEBUG") != nullptr;
        if (occ_dbg) {
            int nb = -1;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(&k_survivor<false>), WAVE, lds_bytes);
            fprintf(stderr, "[occ] k_survivor<false>: %d blocks per CU with %u bytes of LDS, grid %d, punt %d\n", nb, lds_bytes, grid, punt_only);
        }
        CRASS_LAUNCH(k_survivor<false>, dim3(grid), dim3(WAVE), lds_bytes, st, R, P, surv_idx, d_n_surv, n_surv_max,
                           out, dr_chars, dr_stride, ss_pool, ss_pool_cap, d_ss_used, found_flag, seed_hint, lds, punt_only, slot_base, slot_total, punt_list, d_punt_n, redo_list);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Levenshtein / similarity batch: one wave per string pair
// ------------------------------------------------------------------------------------
// lane per pair, bit-parallel; pairs it cannot handle are marked dist = -1 for the wave kernel
__global__ __launch_bounds__(256) void k_lev_batch_lanes(const uint8_t *chars, const uint64_t *a_off, const uint32_t *a_len,
                                                          const uint64_t *b_off, const uint32_t *b_len, uint64_t n_pairs,
                                                          int32_t *dist, float *sim)
{
    uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k >= n_pairs) return;
    const uint8_t *s = chars + a_off[k], *t = chars + b_off[k];
    const int n = (int)a_len[k], m = (int)b_len[k];
    int d = lane_lev_bp(s, n, t, m);
    dist[k] = d;
    if (sim && d >= 0) {
        float max_length = (float)(n > m ? n : m);
        sim[k] = (n < 3 || m < 3) ? 0.0f : (float)(1.0 - (double)((float)d / max_length));
    }
}

__global__ __launch_bounds__(WAVE) void k_lev_batch(const uint8_t *chars, const uint64_t *a_off, const uint32_t *a_len,
                                                     const uint64_t *b_off, const uint32_t *b_len, uint64_t n_pairs,
                                                     int32_t *dist, float *sim, uint32_t row_elems, uint32_t str_bytes)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lv_lds[];
    uint8_t *sa = lv_lds;
    uint8_t *sb = lv_lds + str_bytes;
    uint16_t *rowA = reinterpret_cast<uint16_t *>(lv_lds + 2 * (size_t)str_bytes);
    uint16_t *rowB = rowA + row_elems;
    const int lane = threadIdx.x;
    for (uint64_t k = blockIdx.x; k < n_pairs; k += gridDim.x) {
        int n = (int)a_len[k], m = (int)b_len[k];
        if (dist[k] != -1) continue;                  // already done by the lane kernel
        wave_sync();
        for (int i = lane; i < n; i += WAVE) sa[i] = chars[a_off[k] + i];
        for (int i = lane; i < m; i += WAVE) sb[i] = chars[b_off[k] + i];
        wave_sync();
        int d = wave_lev(sa, n, sb, m, rowA, rowB, lane);
        float s = 0.0f;
        if (sim) s = wave_similarity(sa, n, sb, m, rowA, rowB, lane);
        if (lane == 0) { dist[k] = d; if (sim) sim[k] = s; }
    }
}

hipError_t launch_levenshtein_batch(const uint8_t *chars, const uint64_t *a_off, const uint32_t *a_len,
                                    const uint64_t *b_off, const uint32_t *b_len, uint64_t n_pairs,
                                    int32_t *dist, float *sim, uint32_t max_len, hipStream_t st)
{
    if (n_pairs == 0) return hipSuccess;
    uint32_t str_bytes = (max_len + 16 + 15u) & ~15u;
    uint32_t row_elems = ((max_len + 8) + 7u) & ~7u;
    size_t lds = 2 * (size_t)str_bytes + 2 * (size_t)row_elems * 2;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_lev_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // `dist` is always a device buffer here (engine.cpp allocates it even if the caller wants only sims)
    CRASS_LAUNCH(k_lev_batch_lanes, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, chars, a_off, a_len, b_off, b_len, n_pairs, dist, sim);
    uint64_t grid = n_pairs < 4096 ? n_pairs : 4096;
    CRASS_LAUNCH(k_lev_batch, dim3((unsigned)grid), dim3(WAVE), lds, st, chars, a_off, a_len, b_off, b_len, n_pairs, dist, sim, row_elems, str_bytes);
    return hipGetLastError();
}

} // namespace crass
