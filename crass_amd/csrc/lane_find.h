// lane_find.h — the lane kernel's seed find (k_survivor_lanes, survivor_lanes.hip: ln_find) as a pure function on registers, one
// source for the device and for the host program that checks it against the serial rule (tools/lane_find_main.cpp,
// tests/test_lane_find_host.py).  Plain C++ on the host; under hipcc a __host__ __device__ function whose three primitive
// steps are single gfx950 instructions on the device.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#ifndef CRASS_HD
#ifdef __HIPCC__
#define CRASS_HD __host__ __device__
#else
#define CRASS_HD
#endif
#endif

#ifdef __HIPCC__
#define CRASS_LF_UNROLL _Pragma("unroll")
#else
#define CRASS_LF_UNROLL
#endif

namespace crass {

// the low 32 bits of (hi:lo) >> sh, sh < 32 (v_alignbit_b32)
CRASS_HD inline uint32_t lf_alignbit(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
#endif
}

// One step of the two running counts kept in the halfwords of acc: a halfword of x that is zero (a match) sets its count
// to 0, any other adds 1 — count = (count + 1) * min(x, 1), a packed minimum and a packed multiply-add.  Walked from the
// last candidate down to the first, a count ends as the number of candidates before the first match.
CRASS_HD inline uint32_t lf_step(uint32_t acc, uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // (the minimum as the instruction itself: through the builtin the optimiser knows the result to be 0 or 1 and turns the
    // pair into two compares and two selects per step, with a wait state between each compare and its select)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    uint32_t nz;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(nz) : "v"(x), "v"(0x00010001u));
    const u16x2 z = __builtin_bit_cast(u16x2, nz);
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, acc) * z + z));      // v_pk_mad_u16
#else
    const uint32_t nl = (x & 0xFFFFu) ? 1u : 0u, nh = (x >> 16) ? 1u : 0u;
    return ((((acc & 0xFFFFu) + 1u) * nl) & 0xFFFFu) | (((((acc >> 16) + 1u) * nh) & 0xFFFFu) << 16);
#endif
}

// Step i of 0 .. 31 looks at the candidate offsets 16 (i >> 3) + (i & 7) and that + 8: one funnel shift over the four words
// brings their two 8-mers into the halfwords of a register, one xor-and-mask against the duplicated code tests both.
constexpr int kLaneFindSteps = 32;
// the steps that a window of at most this many candidates needs: offsets 0 .. 48 lie in steps 0 .. 24 (the default window,
// highDR + highSp + w - lowDR - lowSp - w + 1 = 49 candidates)
constexpr int kLaneFindShortNpos = 49, kLaneFindShortSteps = 25;

// smallest t < npos with bases [t, t + plen) == code, else -1.
//   lo, hi   bases 0 .. 63 of the text, base 0 in bits 0-1 of lo (bases past the text: 0)
//   code     the w-mer's 2 * plen bits, plen <= 8
//   npos     candidate offsets 0 .. npos - 1, npos <= 64 - plen + 1 (npos <= 0: -1)
//   all_steps false: only the first kLaneFindShortSteps steps are walked — the caller knows npos <= kLaneFindShortNpos
// An offset beyond 64 - plen sees zero bases shifted in and may "match" a code that ends in A's: it is >= npos, and a match
// at a larger offset never hides one at a smaller offset.
CRASS_HD inline int find_packed_steps(uint64_t lo, uint64_t hi, uint32_t code, int plen, int npos, bool all_steps)
{
    const uint32_t w[5] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 0u};
    const uint32_t m = (1u << (2 * plen)) - 1u;
    const uint32_t mask2 = m | (m << 16), code2 = (code & m) | ((code & m) << 16);
    uint32_t acc = 0;
    if (all_steps) {
CRASS_LF_UNROLL
        for (int i = kLaneFindSteps - 1; i >= kLaneFindShortSteps; i--) {
            const int k = i >> 3, t = i & 7;
            acc = lf_step(acc, (lf_alignbit(w[k + 1], w[k], 2u * (uint32_t)t) ^ code2) & mask2);
        }
    }
CRASS_LF_UNROLL
    for (int i = kLaneFindShortSteps - 1; i >= 0; i--) {
        const int k = i >> 3, t = i & 7;
        acc = lf_step(acc, (lf_alignbit(w[k + 1], w[k], 2u * (uint32_t)t) ^ code2) & mask2);
    }
    // a count of c steps before the first match = offset 16 (c >> 3) + (c & 7), + 8 in the upper halfword; no match: a count
    // of 25 or 32, offset 49 or 64 and beyond — never below npos
    const uint32_t cl = acc & 0xFFFFu, ch = acc >> 16;
    const uint32_t ol = ((cl >> 3) << 4) + (cl & 7u), oh = ((ch >> 3) << 4) + (ch & 7u) + 8u;
    const uint32_t o = ol < oh ? ol : oh;
    return (int)o < npos ? (int)o : -1;
}

// The plain entry point: every step, whatever npos.  The host program checks it; the kernel calls find_packed_steps itself,
// with all_steps false where no lane of the wave has more than kLaneFindShortNpos candidates in its chunk.
CRASS_HD inline int find_packed(uint64_t lo, uint64_t hi, uint32_t code, int plen, int npos)
{
    return find_packed_steps(lo, hi, code, plen, npos, true);
}

} // namespace crass
