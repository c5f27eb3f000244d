// long_light.hip — pass 1, step 2 for gfx950: long reads' light walk (k_long_light, k_long_light_any), which decides the reads
// without an array and hands the others to k_survivor<false> (survivor_wave.hip).  kernels.hip has the map of pass 1's files;
// the helpers shared with the survivor kernels are in search_bits.h.  Compiled as part of survivors.hip.
#include "search_bits.h"
#include <algorithm>

namespace crass {

// ------------------------------------------------------------------------------------
// Long reads, the LIGHT walk.  19 reads in 20 of a long-read set hold no array: their searchCore (libcrispr.cpp:265-395) is a
// walk over ~1 250 seeds of which one or two have a chance copy in range, a two-repeat candidate that the extension rejects, a
// move to another residue class (:390) and more walking.  The full wave kernel (survivor_wave.hip) spends 34 k cycles on such a read — all of
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

} // namespace crass
