// search_bits.h — device functions shared by pass 1's kernel files (kernels.hip; survivor_wave.hip, long_light.hip and
// survivor_lanes.hip, which survivors.hip compiles as one unit): the packed-word code and hint-bit forms of the seed test, the 128-bit piece of a read, and the register
// forms of the run lengths and the bit-parallel edit distance.  Each is defined once, before anything uses it; everything here
// is static and force-inlined unless it says otherwise, and a function used by one file only lives there.
#pragma once
#include "dev_common.h"
#include "comp_table.h"

namespace crass {

static __constant__ CompTable c_comp = make_comp_table();     // reverseComplement table, SeqUtils.cpp:50-59 (one copy per translation unit)

// the w-mer at base p of a read's packed words as one code of 2 w bits (mask = (1 << 2w) - 1); reads one word past p's
static __device__ __forceinline__ uint32_t lds_code(const uint32_t *w, uint32_t p, uint32_t mask)
{
    uint32_t wi = p >> 4, sh = (p & 15u) * 2u;
    uint64_t v = ((uint64_t)w[wi + 1] << 32) | w[wi];
    return (uint32_t)(v >> sh) & mask;
}

// min(halfword, 1) for both halfwords: 0 where the halfword is 0, else 1.  Through the builtin the optimiser turns this into
// two compares, two selects and a permute; the instruction itself is what is wanted.
static __device__ __forceinline__ uint32_t pk_nonzero_u16(uint32_t a)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(0x00010001u));
    return r;
}
typedef uint32_t ff_u32x4 __attribute__((ext_vector_type(4), aligned(4)));      // a row's words, four per load (ff_load_words, k_survivor_lanes)

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

// The every-position form of the scan for one hint word: bit p is set iff the wn-mer at position p has a copy D0 .. D1 further on
// (k_filter_fast_any's test, any window and lattice).  Used by k_hint_filter_any (kernels.hip) and by the light walk k_long_light_any (long_light.hip).
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

// std::string::substr(pos, n) length: throws if pos > size
static __device__ __forceinline__ bool substr_len(int L, uint32_t pos, uint32_t n, uint32_t &len)
{
    if (pos > (uint32_t)L) return false;
    uint32_t avail = (uint32_t)L - pos;
    len = n < avail ? n : avail;
    return true;
}

// leftmost occurrence of the w-mer at `pat` in [begin, end), by the wave — wave_find's contract (survivor_wave.hip:
// PatternMatcher::bmpSearch semantics) on the 2-bit packed copy: a w-mer is one <=18-bit code, so a window compare is
// one LDS word pair + funnel shift per lane instead of w byte compares.  (Not force-inlined.)
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

// bases [start, start + 64) of a read as two 64-bit words (2 bits per base, base `start` in bits 0-1); start >= 0.  Word i of
// the read is w[i * STRIDE]: 1 for a wave's read in LDS (wv_load128), WAVE for a lane's column of it (ln_load128,
// survivor_lanes.hip).  Five independent LDS reads and four funnel shifts; words past the read are whatever the LDS holds
// there: every consumer masks by its own length.
template <int STRIDE>
static __device__ __forceinline__ void load128(const uint32_t *w, int start, uint64_t &lo, uint64_t &hi)
{
    const int wi = start >> 4;
    const uint32_t sh = (uint32_t)(start & 15) * 2u;
    const uint32_t a0 = w[wi * STRIDE], a1 = w[(wi + 1) * STRIDE], a2 = w[(wi + 2) * STRIDE], a3 = w[(wi + 3) * STRIDE], a4 = w[(wi + 4) * STRIDE];
    const uint32_t y0 = __builtin_amdgcn_alignbit(a1, a0, sh), y1 = __builtin_amdgcn_alignbit(a2, a1, sh);
    const uint32_t y2 = __builtin_amdgcn_alignbit(a3, a2, sh), y3 = __builtin_amdgcn_alignbit(a4, a3, sh);
    lo = (uint64_t)y0 | ((uint64_t)y1 << 32); hi = (uint64_t)y2 | ((uint64_t)y3 << 32);
}
static __device__ __forceinline__ void wv_load128(const uint32_t *words, int start, uint64_t &lo, uint64_t &hi) { load128<1>(words, start, lo, hi); }

// A read's words for a wave (k_survivor's and the light walk's prefetch), one 16-byte group per lane and load
// (the words travel 16 bytes per lane and load: a read is word-aligned, not 16-byte aligned, and the hardware takes a
// dword-aligned global_load_dwordx4 — a quarter of the load and LDS-store instructions of the one-word form)
typedef uint32_t sv_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
// group gi (words 4 gi .. 4 gi + 3) of a read of nw words at g; words past the read are 0 and never touched in memory
static __device__ __forceinline__ uint4 sv_load_group(const uint32_t *g, int gi, int nw)
{
    uint4 v; v.x = v.y = v.z = v.w = 0u;
    const int b = 4 * gi;
    if (b + 3 < nw) { const sv_u32x4 t = *reinterpret_cast<const sv_u32x4 *>(g + b); v.x = t.x; v.y = t.y; v.z = t.z; v.w = t.w; }
    else if (b < nw) { v.x = g[b]; if (b + 1 < nw) v.y = g[b + 1]; if (b + 2 < nw) v.z = g[b + 2]; }
    return v;
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

// Bit-parallel distance (see lane_lev_bp, survivor_wave.hip: Hyyro's OSA recurrences with the reference's transposition term restricted to
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

} // namespace crass
