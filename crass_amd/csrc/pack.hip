// pack.hip — the 2-bit packer on the device: concatenated sequence text (one byte per base, reads at arbitrary byte
// offsets) -> the packed read set of include/crass_hip.h, with crass_pack_reads' byte semantics (ingest.cpp).
//
// A pure stream: 1 byte in, 0.25 byte out per base.  A block owns a tile of kPackTileWords consecutive OUTPUT words (so
// every lane stores one aligned 16-byte vector, whatever the reads' lengths); the text those words come from is one
// contiguous span of at most 16 bytes per word, because reads lie back to back in the text and word-aligned in the set.
//   1. every lane resolves its four words: read, word of the read, text position, bases in the word (0 .. 16);
//   2. the block loads the span with ALIGNED 16-byte loads, consecutive lanes consecutive vectors (the span's first and last
//      vector may reach up to 15 bytes beyond it: never into another page, an aligned vector holds a byte of the span);
//      each vector is converted where it was loaded (pack_code4 on its four dwords) and leaves 32 bits of codes and 16
//      "not ACGT" bits in LDS: 6 bytes per 16 of text, so LDS traffic is a third of the text and no byte is touched twice;
//   3. a word whose text starts at byte b of vector v is a funnel shift over the codes of v and v + 1 by 2 b, cut to the
//      bases it holds; its flag is the same shift over the two bit sets;
//   4. a read's flag reaches the 1-bit-per-read mask once per wave and mask word: the lanes that hold a flagged word of a
//      read in that mask word are found by ballot, their bits are OR-ed across the wave and ONE lane issues the atomic
//      (a read's words can lie in several lanes, waves and blocks, so a plain store of a ballot would lose bits).  Sets
//      without exception reads never enter that loop.
#include "pack_launch.h"
#include "devmem.h"
#include <algorithm>

namespace crass {

static constexpr int kPackThreads = 256;
static constexpr uint32_t kPackTileWords = 4 * kPackThreads;
static constexpr uint32_t kPackVecs = kPackTileWords + 4;      // 16-byte vectors of a tile's span: at most kPackTileWords + 1, and the one behind

static __device__ __forceinline__ uint64_t pk_off(const PackJob &J, uint64_t r)
{
    return J.off ? J.off[r] : J.uni_base + r * (uint64_t)J.uni_len;
}
// the last r of [lo, hi] with word_off[r] <= w (word_off[lo] <= w); r == r_end: the word belongs to no read
static __device__ __forceinline__ uint64_t pk_find(const uint64_t *word_off, uint64_t lo, uint64_t hi, uint64_t w)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (word_off[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kPackThreads) void k_pack_text(const PackJob J)
{
    __shared__ uint32_t s_code[kPackVecs];
    __shared__ uint32_t s_bad[kPackVecs];
    __shared__ uint64_t s_span[2];      // text offsets [first, last) of the tile, caller's numbering
    __shared__ uint64_t s_reads[2];     // per-read word offsets: the reads of the tile's first and last word
    const uint32_t tid = threadIdx.x;
    const uint64_t tile0 = (J.w_begin & ~3ull) + (uint64_t)blockIdx.x * kPackTileWords;
    const uint64_t wf = tile0 > J.w_begin ? tile0 : J.w_begin;
    const uint64_t wl = tile0 + kPackTileWords < J.w_end ? tile0 + kPackTileWords : J.w_end;      // the tile's words of this job: [wf, wl), not empty
    if (!J.stride_words) {
        if (tid < 2) s_reads[tid] = pk_find(J.word_off, J.r_begin, J.r_end, tid ? wl - 1 : wf);
        __syncthreads();
    }
    // 1. this lane's four words
    uint64_t rd[4], tpos[4];
    uint32_t valid[4];
    bool mine[4];
    uint64_t r_prev = J.stride_words ? 0 : s_reads[0];
    uint64_t sr = 0, sk = 0;                            // one stride: read and word of the lane's first word (one division per lane)
    if (J.stride_words) { sr = (tile0 + 4u * tid) / J.stride_words; sk = (tile0 + 4u * tid) - sr * J.stride_words; }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint64_t w = tile0 + 4u * tid + q;
        mine[q] = w >= wf && w < wl;
        rd[q] = J.r_end; tpos[q] = 0; valid[q] = 0;
        if (!mine[q]) continue;
        uint64_t r, k;
        if (J.stride_words) {
            r = sr; k = sk + q;
            if (k >= J.stride_words) { k -= J.stride_words; r++; if (k >= J.stride_words) { r += k / J.stride_words; k %= J.stride_words; } }
            if (r > J.r_end) r = J.r_end;
        }
        else { r = pk_find(J.word_off, r_prev, s_reads[1], w); r_prev = r; k = r < J.r_end ? w - J.word_off[r] : 0; }
        rd[q] = r;
        if (r < J.r_end) {
            const uint64_t o0 = pk_off(J, r);
            const uint64_t L = J.off ? J.off[r + 1] - o0 : (uint64_t)J.uni_len;
            const uint64_t kb = 16 * k;
            valid[q] = L > kb ? (uint32_t)(L - kb < 16 ? L - kb : 16) : 0u;
            tpos[q] = o0 + (kb < L ? kb : L);
        } else {
            tpos[q] = pk_off(J, J.r_end);
        }
        if (w == wf) s_span[0] = tpos[q];
        if (w == wl - 1) s_span[1] = tpos[q] + valid[q];
    }
    __syncthreads();
    // 2. the span, converted on the way into LDS
    const uint64_t ts = s_span[0], te = s_span[1];
    const uintptr_t a0 = (uintptr_t)J.text + (uintptr_t)(ts - J.bias);
    const uintptr_t as = a0 & ~(uintptr_t)15;
    const uint32_t n_vec = te > ts ? (uint32_t)((a0 + (uintptr_t)(te - ts) - as + 15) >> 4) : 0u;      // <= kPackTileWords + 1
    const uint4 *src = reinterpret_cast<const uint4 *>(as);
    for (uint32_t i = tid; i < n_vec; i += kPackThreads) {
        const uint4 v = src[i];
        uint32_t b0, b1, b2, b3;
        const uint32_t c0 = pack_code4(v.x, &b0), c1 = pack_code4(v.y, &b1), c2 = pack_code4(v.z, &b2), c3 = pack_code4(v.w, &b3);
        s_code[i] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
        s_bad[i] = b0 | (b1 << 4) | (b2 << 8) | (b3 << 12);
    }
    __syncthreads();
    // 3. the words
    uint32_t word[4], bad[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        word[q] = 0; bad[q] = 0;
        if (!valid[q]) continue;
        const uint32_t o = (uint32_t)((uintptr_t)J.text + (uintptr_t)(tpos[q] - J.bias) - as);
        const uint32_t v = o >> 4, b = o & 15u;
        const uint32_t keep = valid[q] < 16 ? (1u << (2 * valid[q])) - 1u : 0xFFFFFFFFu;
        word[q] = __funnelshift_r(s_code[v], s_code[v + 1], 2 * b) & keep;
        bad[q] = ((s_bad[v] | (s_bad[v + 1] << 16)) >> b) & ((1u << valid[q]) - 1u);
    }
    uint32_t *dst = J.out + tile0 + 4u * tid;
    if (mine[0] && mine[3]) {
        uint4 o4; o4.x = word[0]; o4.y = word[1]; o4.z = word[2]; o4.w = word[3];
        *reinterpret_cast<uint4 *>(dst) = o4;
    } else {                                            // (the one vector at either end of a job that it shares with its neighbour)
#pragma unroll
        for (int q = 0; q < 4; q++) if (mine[q]) dst[q] = word[q];
    }
    // 4. exception reads
    const int lane = (int)(tid & 63u);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        bool pend = bad[q] != 0;
        unsigned long long bal = __ballot(pend);
        while (bal) {
            const int leader = __ffsll(bal) - 1;
            const uint32_t mw_lo = (uint32_t)__shfl((int)(uint32_t)(rd[q] >> 5), leader), mw_hi = (uint32_t)__shfl((int)(uint32_t)(rd[q] >> 37), leader);
            const uint64_t mw = ((uint64_t)mw_hi << 32) | mw_lo;
            const bool now = pend && (rd[q] >> 5) == mw;
            uint32_t bits = now ? 1u << (uint32_t)(rd[q] & 31u) : 0u;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, s);
            if (lane == leader) atomicOr(&J.exc_mask[mw], bits);
            pend = pend && !now;
            bal = __ballot(pend);
        }
    }
}

__global__ __launch_bounds__(256) void k_gather_exc_text(const uint8_t *text, uint64_t bias, const uint64_t *off, uint64_t uni_base, uint32_t uni_len,
                                                         const uint64_t *exc_read, const uint64_t *exc_off, uint64_t n_exc, uint8_t *exc_bytes)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t e = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_exc; e += (uint64_t)gridDim.x * 4) {
        const uint64_t r = exc_read[e];
        const uint8_t *s = text + ((off ? off[r] : uni_base + r * (uint64_t)uni_len) - bias);
        const uint64_t at = exc_off[e], L = exc_off[e + 1] - at;
        for (uint64_t i = lane; i < L; i += 64) exc_bytes[at + i] = s[i];
    }
}

hipError_t launch_pack_text(const PackJob &J, hipStream_t st)
{
    if (J.w_end <= J.w_begin) return hipSuccess;
    const uint64_t span = J.w_end - (J.w_begin & ~3ull);
    const uint64_t tiles = (span + kPackTileWords - 1) / kPackTileWords;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_pack_text, dim3((unsigned)tiles), dim3(kPackThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_gather_exc_text(const uint8_t *text, uint64_t bias, const uint64_t *off, uint64_t uni_base, uint32_t uni_len,
                                  const uint64_t *exc_read, const uint64_t *exc_off, uint64_t n_exc, uint8_t *exc_bytes, hipStream_t st)
{
    if (!n_exc) return hipSuccess;
    const unsigned grid = (unsigned)std::min<uint64_t>((n_exc + 3) / 4, 65536);
    CRASS_LAUNCH(k_gather_exc_text, dim3(grid), dim3(256), 0, st, text, bias, off, uni_base, uni_len, exc_read, exc_off, n_exc, exc_bytes);
    return hipGetLastError();
}

} // namespace crass
