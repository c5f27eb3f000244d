// pack.hip — the 2-bit packer on the device: concatenated sequence text (one byte per base, reads at arbitrary byte
// offsets) -> the packed read set of include/crass_hip.h, with crass_pack_reads' byte semantics (ingest.cpp); and the way
// back, k_fetch_text (below the packer): selected reads of the resident set as text again, forward or reverse-complemented.
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
#include "comp_table.h"
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

// ---- k_fetch_text: the way back.  A stream driven by the OUTPUT: 0.25 byte read, 1 byte written per base ----
// A block owns kFetchTileBytes consecutive output bytes that start on a 16-byte ADDRESS boundary (the output buffer itself may
// start anywhere), a lane one aligned 16-byte vector of them.  The records that meet the tile are found by bisection in
// out_off (two lanes, for the tile's first and last byte), a lane's own first record by bisection between those; a vector
// inside one long read takes one turn of the loop below, a vector over many short or empty records one turn per record that
// has a byte in it (empty records are stepped over by the bisection).
// A turn builds the WHOLE vector as if the record went on for ever on both sides — vector byte t is the record's byte j0 + t —
// and keeps the bytes the record really has:
//   forward:             the 16 codes from base j0 on: a funnel shift over (at most) two packed words; four codes -> four
//                        letters by one byte permute against "ACGT" (the selector = the codes spread to a byte each);
//   reverse complement:  vector byte t is the complement of base L - 1 - j0 - t: the 16 codes from base L - 16 - j0 on, the
//                        permute against "TGCA" (code c -> the complement's letter) with the selector's bytes reversed and the
//                        four dwords in reverse order;
//   exception read:      its raw bytes (exc_bytes; the slot by bisection in exc_read), through c_fcomp under the flag.
// Words are only loaded where the read has one (a caller's attached buffer ends with its last read's last word).
// Every lane stores its vector once: 16 aligned bytes, or — the first and the last vector of the output — its bytes one by one.
static constexpr int kFetchThreads = 256;
static constexpr uint32_t kFetchTileBytes = 16 * kFetchThreads;

static __constant__ CompTable c_fcomp = make_comp_table();      // reverseComplement table (comp_table.h)

// the 16 codes of a read from base j on (j < 0 or beyond the read: codes of no meaning); W: the read's nw words
static __device__ __forceinline__ uint32_t ft_window(const uint32_t *W, int32_t j, int32_t nw)
{
    const int32_t w = j >> 4;                           // (floor: j may be -15 .. -1)
    const uint32_t s = 2u * (uint32_t)(j & 15);
    const uint32_t lo = (w >= 0 && w < nw) ? W[w] : 0u;
    const uint32_t hi = (s && w + 1 >= 0 && w + 1 < nw) ? W[w + 1] : 0u;
    return __funnelshift_r(lo, hi, s);
}
// four codes (8 bits) -> one per byte: a v_perm_b32 selector
static __device__ __forceinline__ uint32_t ft_sel(uint32_t c)
{
    c &= 0xFFu;
    return (c | (c << 6) | (c << 12) | (c << 18)) & 0x03030303u;
}
static __device__ __forceinline__ uint32_t ft_low_bytes(int32_t k)      // the k lowest bytes of a dword, k clamped to 0 .. 4
{
    return k <= 0 ? 0u : (k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u);
}

__global__ __launch_bounds__(kFetchThreads) void k_fetch_text(const FetchJob J)
{
    __shared__ uint64_t s_rec[2];                       // the records of the tile's first and last byte
    const DevReads &R = J.R;
    const uint32_t tid = threadIdx.x;
    // positions count from the aligned address at or below out: the output is [lead, end)
    const uint64_t lead = (uint64_t)((uintptr_t)J.out & 15u), end = lead + J.total;
    const uint64_t tile0 = (uint64_t)blockIdx.x * kFetchTileBytes;
    if (tid < 2) {
        const uint64_t tile_end = tile0 + kFetchTileBytes < end ? tile0 + kFetchTileBytes : end;
        const uint64_t p = tid ? tile_end - 1 : (tile0 > lead ? tile0 : lead);      // (the tile holds a byte of the output: the grid ends with it)
        s_rec[tid] = pk_find(J.out_off, 0, J.n - 1, p - lead);
    }
    __syncthreads();
    const uint64_t v0 = tile0 + 16u * tid;
    const uint64_t a = v0 > lead ? v0 : lead, b = v0 + 16 < end ? v0 + 16 : end;      // this lane's bytes: [a, b)
    if (a >= b) return;
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    const int64_t vrel = (int64_t)v0 - (int64_t)lead;   // output offset of vector byte 0 (negative in the first vector of an unaligned output)
    const uint64_t stop = b - lead;
    uint64_t pos = a - lead;
    uint64_t k = pk_find(J.out_off, s_rec[0], s_rec[1], pos);
    for (;;) {
        const uint64_t o0 = J.out_off[k], o1 = J.out_off[k + 1];      // o0 <= pos < o1
        const int32_t L = (int32_t)(o1 - o0);
        const int32_t j0 = (int32_t)(vrel - (int64_t)o0);
        const int32_t t0 = j0 < 0 ? -j0 : 0, t1 = L - j0 < 16 ? L - j0 : 16;      // the record's bytes of the vector: [t0, t1)
        const uint64_t r = J.idx[k];
        const bool rc = J.rc && J.rc[k];
        uint32_t x[4] = {0u, 0u, 0u, 0u};
        if (!((R.exc_mask[r >> 5] >> (uint32_t)(r & 31u)) & 1u)) {
            const uint32_t *W = R.packed + (R.stride_words ? r * (uint64_t)R.stride_words : R.word_off[r]);
            const int32_t nw = (L + 15) >> 4;
            if (!rc) {
                const uint32_t c = ft_window(W, j0, nw);
#pragma unroll
                for (int q = 0; q < 4; q++) x[q] = __builtin_amdgcn_perm(0x54474341u, 0x54474341u, ft_sel(c >> (8 * q)));      // "ACGT"
            } else {
                const uint32_t c = ft_window(W, L - 16 - j0, nw);
#pragma unroll
                for (int q = 0; q < 4; q++) x[q] = __builtin_amdgcn_perm(0x41434754u, 0x41434754u, __builtin_bswap32(ft_sel(c >> (8 * (3 - q)))));      // "TGCA"
            }
        } else {
            uint64_t lo = 0, hi = R.n_exc - 1;          // the read's slot: exc_read is ascending and holds r
            while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (R.exc_read[mid] < r) lo = mid + 1; else hi = mid; }
            const uint8_t *src = R.exc_bytes + R.exc_off[lo];
#pragma unroll
            for (int t = 0; t < 16; t++) {
                if (t < t0 || t >= t1) continue;
                const uint32_t by = rc ? (uint32_t)c_fcomp.v[src[L - 1 - j0 - t] & 127] : (uint32_t)src[j0 + t];
                x[t >> 2] |= by << (8 * (t & 3));
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] |= x[q] & ft_low_bytes(t1 - 4 * q) & ~ft_low_bytes(t0 - 4 * q);
        pos = o1;
        if (pos >= stop) break;
        k = pk_find(J.out_off, k + 1, s_rec[1], pos);
    }
    uint8_t *dst = J.out + vrel;                        // 16-byte aligned (up to 15 bytes below out in the first vector: those are not stored)
    if (a == v0 && b == v0 + 16) {
        uint4 o4; o4.x = acc[0]; o4.y = acc[1]; o4.z = acc[2]; o4.w = acc[3];
        *reinterpret_cast<uint4 *>(dst) = o4;
    } else {                                            // (the output's first or last vector)
        const uint32_t ta = (uint32_t)(a - v0), tb = (uint32_t)(b - v0);
#pragma unroll
        for (uint32_t t = 0; t < 16; t++) if (t >= ta && t < tb) dst[t] = (uint8_t)(acc[t >> 2] >> (8 * (t & 3)));
    }
}

hipError_t launch_fetch_text(const FetchJob &J, hipStream_t st)
{
    if (!J.n || !J.total) return hipSuccess;
    const uint64_t span = (uint64_t)((uintptr_t)J.out & 15u) + J.total;
    const uint64_t tiles = (span + kFetchTileBytes - 1) / kFetchTileBytes;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_fetch_text, dim3((unsigned)tiles), dim3(kFetchThreads), 0, st, J);
    return hipGetLastError();
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
