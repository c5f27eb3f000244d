// survivor_lanes.hip — pass 1, step 2 (fast path) for gfx950: the lane-per-read survivor search (k_survivor_lanes), its QC
// task pool and launch.  kernels.hip has the map of pass 1's files; the register forms it shares with the wave kernel and the
// light walk (ln_lev_regs, ln_run_up / ln_run_down, load128) are in search_bits.h.  Compile with -ffp-contract=off:
// qcFoundRepeats' float evaluation order is part of the parity contract.  Compiled as part of survivors.hip.
#include "search_bits.h"
#include "lane_find.h"

namespace crass {

// ------------------------------------------------------------------------------------
// pass 1, step 2 (fast path): the same searchCore, one read per LANE.
//
// The wave-per-read kernel (survivor_wave.hip) spends most of its issue slots with one or two useful lanes
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
static __device__ __forceinline__ void ln_load128(const LaneRead &h, int start, uint64_t &lo, uint64_t &hi) { load128<WAVE>(h.w, start, lo, hi); }

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

} // namespace crass
