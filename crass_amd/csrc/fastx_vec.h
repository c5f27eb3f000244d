// fastx_vec.h — what the device kernels over raw FASTA / FASTQ bytes share: the tile's size, a lane's aligned 16-byte vector with
// its byte classes and line starts (fastx_scan.hip, fastx_wrapped.hip), and the block scans: 32-bit (those two) and 64-bit
// (fastx_wrapped.hip, fastx_lines.hip, fastx_hid.hip).  Device code: only .hip files include this.
#pragma once
#include "fastx_launch.h"
#include "devmem.h"

namespace crass {

static constexpr int kFxThreads = 256;
static constexpr uint32_t kFxTileBytes = 16 * kFxThreads;
static constexpr int kFxScanThreads = 1024;

// a lane's vector: the bytes and, 16 bits each, what they are (bit j: byte j; invalid bytes are in no class)
struct FxVec { uint32_t w[4]; uint32_t valid, nl, ls, gt, at, pl, del, gr; };

static __device__ __forceinline__ void fx_load(const FxJob &J, uint64_t q0, FxVec &V)
{
    const uint64_t lead = J.lead, end = lead + J.n;      // the input in aligned space: [lead, end)
    uint32_t valid = 0;
    if (q0 + 16 > lead && q0 < end) {
        const uint32_t lo = q0 < lead ? (uint32_t)(lead - q0) : 0u;
        const uint32_t hi = end - q0 < 16 ? (uint32_t)(end - q0) : 16u;
        valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    }
    const uint8_t *a = reinterpret_cast<const uint8_t *>((uintptr_t)J.bytes - (uintptr_t)lead + (uintptr_t)q0);      // 16-byte aligned
    V.w[0] = V.w[1] = V.w[2] = V.w[3] = 0u;
    if (valid == 0xFFFFu) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a);
        V.w[0] = v.x; V.w[1] = v.y; V.w[2] = v.z; V.w[3] = v.w;
    } else if (valid) {                                  // (the input's first and last vector)
#pragma unroll
        for (int j = 0; j < 16; j++) if ((valid >> j) & 1u) V.w[j >> 2] |= (uint32_t)a[j] << (8 * (j & 3));
    }
    const FxClass4 c0 = fx_class4(V.w[0]), c1 = fx_class4(V.w[1]), c2 = fx_class4(V.w[2]), c3 = fx_class4(V.w[3]);
    V.valid = valid;
    V.nl = (c0.nl | (c1.nl << 4) | (c2.nl << 8) | (c3.nl << 12)) & valid;
    V.gt = (c0.gt | (c1.gt << 4) | (c2.gt << 8) | (c3.gt << 12)) & valid;
    V.at = (c0.at | (c1.at << 4) | (c2.at << 8) | (c3.at << 12)) & valid;
    V.pl = (c0.plus | (c1.plus << 4) | (c2.plus << 8) | (c3.plus << 12)) & valid;
    V.del = (c0.del | (c1.del << 4) | (c2.del << 8) | (c3.del << 12)) & valid;
    V.gr = (c0.graph | (c1.graph << 4) | (c2.graph << 8) | (c3.graph << 12)) & valid;
    // line starts: file position 0, and every valid byte behind a '\n' (the byte in front of the vector: the lane before, or —
    // a wave's first lane — one byte load; it is inside the input)
    uint32_t prev = (uint32_t)__shfl_up((int)(V.nl >> 15), 1);
    if ((threadIdx.x & 63u) == 0) prev = (q0 > lead && q0 - 1 < end) ? (uint32_t)fx_is_nl(a[-1]) : 0u;
    V.ls = (((V.nl << 1) | (prev & 1u)) & 0xFFFFu) & valid;
    if (lead >= q0 && lead < q0 + 16) V.ls |= (1u << (uint32_t)(lead - q0)) & valid;
}

// exclusive prefix sum of v over the block's NW waves; *total: the block's sum.  s_w: NW words of LDS, free again on return
template <int NW> static __device__ __forceinline__ uint32_t fx_scan_add(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, off); if (lane >= off) incl += y; }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) { const uint32_t s = s_w[k]; if (k < wv) base += s; all += s; }
    __syncthreads();
    *total = all;
    return base + incl - v;
}
// the same with max: the largest v of the threads BEFORE this one (0: none); *total: the block's largest
template <int NW> static __device__ __forceinline__ uint32_t fx_scan_max(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, off); if (lane >= off && y > incl) incl = y; }
    if (lane == 63) s_w[wv] = incl;
    uint32_t excl = (uint32_t)__shfl_up((int)incl, 1);
    if (lane == 0) excl = 0u;
    __syncthreads();
    uint32_t all = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) { const uint32_t s = s_w[k]; if (k < wv && s > excl) excl = s; if (s > all) all = s; }
    __syncthreads();
    *total = all;
    return excl;
}
static __device__ __forceinline__ uint32_t fx_wave_sum(uint32_t v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s);
    return v;
}

// ---- the 64-bit scans (a shuffle moves 32 bits: a value travels as its two halves).  Of unsigned values, so 0 is "nothing yet"
// for the sum and for the maximum alike ----
struct FxAdd64 { static __device__ __forceinline__ uint64_t of(uint64_t a, uint64_t b) { return a + b; } };
struct FxMax64 { static __device__ __forceinline__ uint64_t of(uint64_t a, uint64_t b) { return b > a ? b : a; } };

static __device__ __forceinline__ uint64_t fx_shfl_up64(uint64_t v, int s)
{
    const uint32_t a = (uint32_t)__shfl_up((int)(uint32_t)v, s), b = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), s);
    return ((uint64_t)b << 32) | a;
}
static __device__ __forceinline__ uint64_t fx_shfl_xor64(uint64_t v, int s)
{
    const uint32_t a = (uint32_t)__shfl_xor((int)(uint32_t)v, s), b = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s);
    return ((uint64_t)b << 32) | a;
}
// the wave's v under Op, in every lane
template <class Op> static __device__ __forceinline__ uint64_t fx_wave_all64(uint64_t v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = Op::of(v, fx_shfl_xor64(v, s));
    return v;
}
static __device__ __forceinline__ uint64_t fx_wave_sum64(uint64_t v) { return fx_wave_all64<FxAdd64>(v); }
// the block's sum of v over its NW waves, in every lane.  sh: NW words of LDS; safe to call again and again on the same sh
template <int NW> static __device__ __forceinline__ uint64_t fx_block_sum64(uint64_t v, uint64_t *sh)
{
    v = fx_wave_sum64(v);
    __syncthreads();                                    // (sh may still be read from the call before)
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t s = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) s += sh[w];
    return s;
}
// what the lanes in front of this one hold in v, under Op (the exclusive prefix over the block; 0: none); *total: the whole
// block's.  sh as above, with the same barriers
template <int NW, class Op> static __device__ __forceinline__ uint64_t fx_block_prefix64(uint64_t v, uint64_t *sh, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const uint64_t o = fx_shfl_up64(inc, s); if (lane >= (uint32_t)s) inc = Op::of(inc, o); }
    uint64_t before = fx_shfl_up64(inc, 1);
    if (lane == 0) before = 0;
    __syncthreads();                                    // (sh may still be read from the call before)
    if (lane == 63u) sh[wave] = inc;
    __syncthreads();
    uint64_t all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)NW; w++) { const uint64_t s = sh[w]; if (w < wave) before = Op::of(s, before); all = Op::of(all, s); }
    *total = all;
    return before;
}
// the one-block top step of a three-launch scan, by the block's NW waves: a[0, n) in place, 64 NW values a step with what the
// steps before came to in front.  a[t] becomes Op over a[0, t) — with INCL over a[0, t] —; returned: Op over all of them, in every
// lane.  Every lane of the block calls it (the same trip count in each)
template <int NW, class Op, bool INCL> static __device__ __forceinline__ uint64_t fx_top_scan64(uint64_t *a, uint64_t n, uint64_t *sh)
{
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < n; t0 += 64 * NW) {
        const uint64_t t = t0 + threadIdx.x;
        const uint64_t v = t < n ? a[t] : 0;
        uint64_t total;
        uint64_t r = Op::of(carry, fx_block_prefix64<NW, Op>(v, sh, &total));
        if (INCL) r = Op::of(r, v);
        if (t < n) a[t] = r;
        carry = Op::of(carry, total);
    }
    return carry;
}

} // namespace crass
