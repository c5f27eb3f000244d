// survivor_wave.hip — pass 1, step 2 for gfx950: the wave-per-read survivor search (k_survivor: searchCore / scanRight /
// extendPreRepeat / qcFoundRepeats / DRLowLexi of one read, byte for byte), its LDS layouts and launch, and the Levenshtein
// batch, which is built on the same wave_lev / lane_lev_bp.  The phase counters (PROF_* / PF_*, CRASS_SURV_PROF) are this
// kernel's.  kernels.hip has the map of pass 1's files and the reference citations; the helpers shared with the light walk and
// the lane kernel are in search_bits.h.  Compile with -ffp-contract=off: qcFoundRepeats' float evaluation order is part of the
// parity contract.  Compiled as part of survivors.hip, with long_light.hip and survivor_lanes.hip (the reason is there).
#include "search_bits.h"
#include <algorithm>

namespace crass {

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

static __device__ __forceinline__ int rh_find(const RH &h, int begin, int end, int pat, int plen, int lane)
{
    if (h.words) return wave_find_packed(h.words, h.cmask, begin, end, pat, plen, lane);
    return wave_find(h.seq, begin, end, pat, plen, lane);
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

// The byte-wise consumers (extendPreRepeat's column votes, the QC's string comparisons, DRLowLexi) read the bases around the
// repeats found so far, never far from them — a packed read's ASCII copy is expanded for that REGION when they are entered,
// not for the whole read when it is loaded (a 10 kbp read: 10 KB of LDS writes per read against 2.5 KB for the packed words;
// 61 % of random 10 kbp reads meet a candidate, which covers a few hundred bases).  kAscPad bounds how far the consumers
// reach beyond the first repeat's start / the last one's end: one repeat spacing (highDR + highSp, 97 by default) for the
// extensions; RH::asc_pad = that + 32.
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

// ------------------------------------------------------------------------------------
// Packed reads in the wave kernel: scanRight, extendPreRepeat and the QC's edit distances on the 2-bit words in LDS — no
// ASCII window, no per-base LDS round trips.  One long read costs the wave (phase counters, CRASS_SURV_PROF, 1 M x 10 kbp):
// an array read 234 k cycles, of which the QC 128 k (two dependent LDS byte reads per DP column and lane), the scanRight chain
// 52 k (38 finds x {two LDS round trips + a ballot + two fenced list appends}), the extension 31 k (a lane per COLUMN walks the
// 36 repeats, two dependent LDS reads each); a read without an array 27 k, 4.3 k of them a two-repeat extension.  The forms
// below keep the reference's decisions and arithmetic (libcrispr.cpp:170-263, 520-772, 869-1029) and change what a lane holds.
// ------------------------------------------------------------------------------------
// (wv_load128, search_bits.h: bases [start, start + 64) of the read as two 64-bit words)
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

// extendPreRepeat (libcrispr.cpp:520-772) on the packed words.  Two repeats: the closed form of the lane kernel (ln_extend2, survivor_lanes.hip:
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
static __device__ uint32_t extend_pre_repeat(RH &h, int searchWindowLength, int minSpacerLength, int lane)
{
    // packed reads with at most 64 repeats: on the 2-bit words, no ASCII window (defined with the other packed forms above)
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

// getStringSimilarity (PatternMatcher.cpp:197-204) of read[s0, s0+n) and read[t0, t0+m), both <= 64 bases, on the packed words:
// ten independent LDS reads, then the bit-parallel distance runs on registers (ln_lev_regs, search_bits.h: the lane kernel's form)
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

// words of the read a wave works on NEXT, requested while it searches the current one (wave-per-read kernel, long reads:
// a 10 kbp read is ten dependent rounds of loads per lane otherwise — 5.0 of the kernel's 12.3 ms at 1 M x 10 kbp)
#define SV_PREFETCH_WORDS 12                      // per lane: reads up to 12 * 64 * 16 = 12 288 bases are covered completely
#define SV_PREFETCH_HINTS (SV_PREFETCH_WORDS / 4)  // 64-bit hint words per lane for the same reads (one bit per position)
#define SV_PREFETCH_VEC (SV_PREFETCH_WORDS / 4)
struct ReadPrefetch {
    uint4 v[SV_PREFETCH_VEC];                     // lane's 16-byte groups lane, lane + 64, ...: words 4 g .. 4 g + 3
    uint64_t hw[SV_PREFETCH_HINTS];
    uint64_t r;                                   // the read these words belong to (~0: none)
};
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
