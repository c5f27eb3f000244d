// sinks.hip — ordered compaction and hand-off (gfx950): what stands between a search kernel's per-read answers and the
// blobs the host reads.  The exception bit mask and the found flags, the device -> pinned host copy kernel, bit mask ->
// ascending index list (three kernels, or one with decoupled look-back), pass 1's gather of the found records with the
// de-duplication of their DR strings, and pass 2's packing of the valid hits.
#include "dev_common.h"
#include <algorithm>

namespace crass {

// ------------------------------------------------------------------------------------
// exception bit mask
// ------------------------------------------------------------------------------------
__global__ void k_build_exc_mask(const uint64_t *exc_read, uint64_t n_exc, uint32_t *exc_mask)
{
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < n_exc) {
        uint64_t r = exc_read[i];
        atomicOr(&exc_mask[r >> 5], 1u << (r & 31));
    }
}

__global__ void k_mark_found(const uint64_t *idx, uint64_t n, const uint64_t *header_id, uint8_t *found_flag)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < n) { const uint64_t r = idx[i]; found_flag[header_id ? header_id[r] : r] = 1; }
}
hipError_t launch_mark_found(const uint64_t *idx, uint64_t n, const uint64_t *header_id, uint8_t *found_flag, hipStream_t st)
{
    if (!n) return hipSuccess;
    CRASS_LAUNCH(k_mark_found, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, idx, n, header_id, found_flag);
    return hipGetLastError();
}

// k_mark_found over a list made on the device (the answers of crass_hip_fastx_names_find_device): entries equal to kSkip, names
// nobody here carries, are passed over; any other entry >= n_reads marks nothing and sets *bad.  found_flag == nullptr: the
// check alone (crass_hip_recruit_found marks only a list without a bad entry).
__global__ void k_mark_found_skip(const uint64_t *idx, uint64_t n, uint64_t n_reads, const uint64_t *header_id, uint8_t *found_flag, uint32_t *bad)
{
    constexpr uint64_t kSkip = ~0ull;                   // CRASS_NAME_NOT_FOUND
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t r = idx[i];
    if (r == kSkip) return;
    if (r >= n_reads) { *bad = 1u; return; }
    if (found_flag) found_flag[header_id ? header_id[r] : r] = 1;
}
hipError_t launch_mark_found_skip(const uint64_t *idx, uint64_t n, uint64_t n_reads, const uint64_t *header_id, uint8_t *found_flag, uint32_t *bad,
                                  hipStream_t st)
{
    if (!n) return hipSuccess;
    if ((n + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_mark_found_skip, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, idx, n, n_reads, header_id, found_flag, bad);
    return hipGetLastError();
}

// Device -> pinned host copy by a handful of workgroups (the link is the bound: ~55 GB/s needs a few hundred stores in
// flight, not a chip): the fall-back of the DMA-engine copy (sdma.cpp).  Like the runtime's blit kernel it costs the kernels
// of the other stream its own duration — PCIe stores from shader waves do, however few waves issue them and on however
// many XCDs (profiles/NOTES_r03.md §9) — so the engine orders it behind the merge kernels.
__global__ __launch_bounds__(256) void k_copy_to_host(const uint4 *src, uint4 *dst, uint64_t n16, const uint8_t *src_tail, uint8_t *dst_tail, uint32_t n_tail)
{
    const uint64_t nth = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n16; i += nth) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x < n_tail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];
}
hipError_t launch_copy_to_host(const void *d_src, void *h_dst, uint64_t bytes, hipStream_t st)
{
    if (!bytes) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(h_dst)) & 15u) return hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st);
    const uint64_t n16 = bytes / 16;
    const unsigned blocks = (unsigned)std::min<uint64_t>(32, (n16 + 255) / 256 + 1);
    CRASS_LAUNCH(k_copy_to_host, dim3(blocks), dim3(256), 0, st, static_cast<const uint4 *>(d_src), static_cast<uint4 *>(h_dst), n16,
                 static_cast<const uint8_t *>(d_src) + n16 * 16, static_cast<uint8_t *>(h_dst) + n16 * 16, (uint32_t)(bytes & 15u));
    return hipGetLastError();
}

hipError_t launch_build_exc_mask(const uint64_t *exc_read, uint64_t n_exc, uint32_t *exc_mask, hipStream_t st)
{
    if (!n_exc) return hipSuccess;
    CRASS_LAUNCH(k_build_exc_mask, dim3((unsigned)((n_exc + 255) / 256)), dim3(256), 0, st, exc_read, n_exc, exc_mask);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// ordered compaction: bit mask -> ascending list of set-bit indices
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mask_count(const uint64_t *mask, uint64_t n_words, uint64_t n_bits,
                                                     uint32_t *word_prefix, uint32_t *block_sums)
{
    __shared__ uint32_t sh[256];
    uint64_t wi = blockIdx.x * 256ull + threadIdx.x;
    uint32_t c = 0;
    if (wi < n_words) {
        uint64_t m = mask[wi];
        uint64_t rem = n_bits - wi * 64;
        if (rem < 64) m &= (1ull << rem) - 1ull;
        c = (uint32_t)__popcll(m);
    }
    sh[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        uint32_t v = (threadIdx.x >= (unsigned)off) ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    if (wi < n_words) word_prefix[wi] = sh[threadIdx.x] - c;
    if (threadIdx.x == 255) block_sums[blockIdx.x] = sh[255];
}

__global__ __launch_bounds__(1024) void k_block_scan(uint32_t *block_sums, uint32_t n_blocks, uint32_t *d_count, uint32_t *zero_a, uint32_t n_a, uint32_t *zero_b, uint32_t n_b)
{
    // counters the NEXT stage accumulates into are cleared here instead of by their own fill launches
    if (threadIdx.x < n_a) zero_a[threadIdx.x] = 0u;
    if (threadIdx.x < n_b) zero_b[threadIdx.x] = 0u;

    __shared__ uint32_t sh[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_blocks; base += 1024) {
        uint32_t i = base + threadIdx.x;
        uint32_t c = (i < n_blocks) ? block_sums[i] : 0;
        sh[threadIdx.x] = c;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            uint32_t v = (threadIdx.x >= (unsigned)off) ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += v;
            __syncthreads();
        }
        uint32_t excl = sh[threadIdx.x] - c + carry;
        if (i < n_blocks) block_sums[i] = excl;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *d_count = carry;
}

__global__ __launch_bounds__(256) void k_mask_scatter(const uint64_t *mask, uint64_t n_words, uint64_t n_bits,
                                                       const uint32_t *word_prefix, const uint32_t *block_sums,
                                                       uint64_t *out_idx, uint64_t out_cap)
{
    uint64_t wi = blockIdx.x * 256ull + threadIdx.x;
    if (wi >= n_words) return;
    uint64_t m = mask[wi];
    uint64_t rem = n_bits - wi * 64;
    if (rem < 64) m &= (1ull << rem) - 1ull;
    uint64_t o = (uint64_t)block_sums[blockIdx.x] + word_prefix[wi];
    while (m) {
        int b = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        if (o < out_cap) out_idx[o] = wi * 64 + b;
        o++;
    }
}

// ---- single-pass form: decoupled look-back over tiles of 1024 mask words ----
static __device__ __forceinline__ unsigned long long lb_pack(uint32_t epoch, uint32_t flag, uint32_t value)
{
    return ((unsigned long long)epoch << 34) | ((unsigned long long)flag << 32) | value;
}
// Exclusive prefix of this tile's total over the tiles before it.  Called by every thread of the block
// (one __syncthreads inside); wave 0 does the look-back, 64 predecessor tiles per step.
static __device__ uint32_t lb_exclusive_prefix(const Lookback &lb, uint32_t tile, uint32_t total)
{
    __shared__ uint32_t excl_sh;
    if (threadIdx.x < 64) {
        const int lane = (int)threadIdx.x;
        if (lane == 0)
            __hip_atomic_store(&lb.status[tile], lb_pack(lb.epoch, tile == 0 ? 2u : 1u, total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t excl = 0;
        int t = (int)tile - 1;                           // wave-uniform: this step looks at tiles t, t-1, ..., t-63
        while (t >= 0) {
            const int idx = t - lane;
            uint32_t flag = 2u, val = 0u;                // tiles before tile 0: an empty prefix
            if (idx >= 0) {
                flag = 0u;
                for (uint32_t spins = 0; spins < (1u << 24); spins++) {
                    const unsigned long long w = __hip_atomic_load(&lb.status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((uint32_t)(w >> 34) == lb.epoch && ((w >> 32) & 3ull) != 0ull) { flag = (uint32_t)(w >> 32) & 3u; val = (uint32_t)w; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (flag == 0u) { *lb.fail = 1u; flag = 2u; }               // gave up (pinned host word): terminate, the host reports it
            }
            const unsigned long long pm = __ballot(flag == 2u);
            const int stop = pm ? __ffsll(pm) - 1 : 64;  // nearest tile whose inclusive prefix is known
            uint32_t v = lane <= stop ? val : 0u;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
            excl += v;
            if (pm) break;
            t -= 64;
        }
        if (lane == 0) {
            if (tile != 0) __hip_atomic_store(&lb.status[tile], lb_pack(lb.epoch, 2u, excl + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            excl_sh = excl;
        }
    }
    __syncthreads();
    return excl_sh;
}
// A tile id per block, in start order.  n_act blocks of the launch call this (every block computes the same n_act; the
// others have returned before): the block that draws the last ticket puts the counter back to zero for the next launch — by
// then every other ticket of this launch has been drawn.  (The counter is ONE word for all launches of a context's stream.
// Returning atomics on one address retire every 20-30 ns on this part however many CUs issue them — the whole cost of a
// look-back kernel over a few thousand tiles, rocprofv3 round 4: 1 526 tiles of the read mask 32 us, 4 950 mostly EMPTY
// tiles of the candidate list 50 us — so tiles are fat, and tiles past a device-side count draw no ticket at all.)
static __device__ uint32_t lb_tile_id(const Lookback &lb, uint32_t n_act)
{
    __shared__ uint32_t tile_sh;
    if (threadIdx.x == 0) {
        const uint32_t t = atomicAdd(lb.ticket, 1u);
        if (t + 1u >= n_act) __hip_atomic_store(lb.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tile_sh = t;
    }
    __syncthreads();
    return tile_sh;
}
// exclusive prefix of v over the T threads of the block; *total = block sum
template <int T>
static __device__ uint32_t block_scan_t(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t wsum[T / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int k = 0; k < T / 64; k++) { const uint32_t s = wsum[k]; if (k < wv) base += s; all += s; }
    *total = all;
    return base + incl - v;
}

// T threads x W consecutive mask words per tile: 1024 x 4 for the masks over all reads (few, fat tiles: the ticket is the
// kernel's cost), 256 x 1 for the short dense masks of the later stages (more blocks for the per-word scatter loops)
template <int T, int W>
__global__ __launch_bounds__(T) void k_mask_compact_lb(const uint64_t *mask, uint64_t n_words, uint64_t n_bits, uint32_t *word_prefix,
                                                        uint32_t *block_sums, uint64_t *out_idx, uint64_t out_cap, uint32_t *d_count,
                                                        uint32_t *zero_a, uint32_t n_a, uint32_t *zero_b, uint32_t n_b, Lookback lb,
                                                        uint32_t n_tiles)
{
    const uint32_t tile = lb_tile_id(lb, n_tiles);
    if (tile == 0) {                                    // counters the NEXT stage accumulates into
        if (threadIdx.x < n_a) zero_a[threadIdx.x] = 0u;
        if (threadIdx.x < n_b) zero_b[threadIdx.x] = 0u;
    }
    const uint64_t w0 = ((uint64_t)tile * T + threadIdx.x) * W;
    uint64_t m[W];
    uint32_t cnt = 0;
#pragma unroll
    for (int q = 0; q < W; q++) {
        const uint64_t wi = w0 + q;
        m[q] = 0;
        if (wi < n_words) {
            m[q] = mask[wi];
            const uint64_t rem = n_bits - wi * 64;
            if (rem < 64) m[q] &= (1ull << rem) - 1ull;
        }
        cnt += (uint32_t)__popcll(m[q]);
    }
    uint32_t total;
    const uint32_t in_tile = block_scan_t<T>(cnt, &total);
    const uint32_t excl = lb_exclusive_prefix(lb, tile, total);
    if (tile == n_tiles - 1 && threadIdx.x == 0) *d_count = excl + total;
    uint64_t o = (uint64_t)excl + in_tile;
#pragma unroll
    for (int q = 0; q < W; q++) {
        const uint64_t wi = w0 + q;
        if (wi >= n_words) break;
        if (word_prefix) {                              // same meaning as the three-kernel form: block_sums[w >> 8] + word_prefix[w]
            word_prefix[wi] = (uint32_t)o;
            if ((wi & 255u) == 0) block_sums[wi >> 8] = 0u;
        }
        uint64_t mm = m[q];
        while (mm) {
            const int b = __ffsll((unsigned long long)mm) - 1;
            mm &= mm - 1;
            if (o < out_cap) out_idx[o] = wi * 64 + b;
            o++;
        }
    }
}

// element-wise form: tiles of 4096 elements, 1024 threads x 4 consecutive elements (few, fat tiles keep the look-back
// to one or two steps).  cnt = flagged elements of this thread; returns the rank of the thread's first flagged element
// among all flagged elements before it; *upto = flagged elements up to and including this tile.
static constexpr uint32_t kLbElemsPerTile = 4096;
static __device__ uint32_t lb_rank4(const Lookback &lb, uint32_t tile, uint32_t cnt, uint32_t *upto)
{
    uint32_t all;
    const uint32_t in_tile = block_scan_t<1024>(cnt, &all);
    const uint32_t excl = lb_exclusive_prefix(lb, tile, all);
    *upto = excl + all;
    return excl + in_tile;
}

hipError_t launch_compact(const uint64_t *mask, uint64_t n_words, uint64_t n_bits, uint32_t *word_prefix,
                          uint32_t *block_sums, uint64_t *out_idx, uint64_t out_cap, uint32_t *d_count, hipStream_t st,
                          uint32_t *zero_a, uint32_t n_a, uint32_t *zero_b, uint32_t n_b, const Lookback *lb)
{
    if (lb && n_words) {
        // (the caller reserved ceil(n_words / lookback_tile_words(n_words)) tickets)
        const uint32_t tw = lookback_tile_words(n_words);
        const uint32_t n_tiles = (uint32_t)((n_words + tw - 1) / tw);
        if (tw == 256)
            CRASS_LAUNCH((k_mask_compact_lb<256, 1>), dim3(n_tiles), dim3(256), 0, st, mask, n_words, n_bits, word_prefix, block_sums, out_idx, out_cap,
                               d_count, zero_a, n_a, zero_b, n_b, *lb, n_tiles);
        else
            CRASS_LAUNCH((k_mask_compact_lb<1024, 4>), dim3(n_tiles), dim3(1024), 0, st, mask, n_words, n_bits, word_prefix, block_sums, out_idx, out_cap,
                               d_count, zero_a, n_a, zero_b, n_b, *lb, n_tiles);
        return hipGetLastError();
    }
    if (n_words == 0) {
        if (n_a) (void)hipMemsetAsync(zero_a, 0, 4 * (size_t)n_a, st);
        if (n_b) (void)hipMemsetAsync(zero_b, 0, 4 * (size_t)n_b, st);
        return hipMemsetAsync(d_count, 0, 4, st);
    }
    unsigned nb = (unsigned)((n_words + 255) / 256);
    CRASS_LAUNCH(k_mask_count, dim3(nb), dim3(256), 0, st, mask, n_words, n_bits, word_prefix, block_sums);
    CRASS_LAUNCH(k_block_scan, dim3(1), dim3(1024), 0, st, block_sums, nb, d_count, zero_a, n_a, zero_b, n_b);
    CRASS_LAUNCH(k_mask_scatter, dim3(nb), dim3(256), 0, st, mask, n_words, n_bits, word_prefix, block_sums, out_idx, out_cap);
    return hipGetLastError();
}

// ---- device-side gather of the found records (fast path: short reads, slot-mode pool) ----
// mask of slots with found != 0; the worst error code is max-reduced into *d_err
__global__ __launch_bounds__(256) void k_found_mask(const SurvOut *out, const uint32_t *d_n, uint64_t n, uint64_t *mask, uint32_t *d_err,
                                                     unsigned long long *dd_keys, uint32_t *dd_first, uint32_t dd_size)
{
    const uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    // the de-duplication table of the next stage is cleared on the way (saves its own launch)
    for (uint64_t i = s; i < dd_size; i += (uint64_t)gridDim.x * blockDim.x) { dd_keys[i] = 0ull; dd_first[i] = 0xFFFFFFFFu; }
    bool f = false;
    if (s < n && s < (uint64_t)*d_n) {                  // slots past the device-side count were never written
        const SurvOut o = out[s];
        f = o.found != 0;
        if (o.err) atomicMax(d_err, (uint32_t)o.err);
    }
    const uint64_t m = __ballot(f);
    if ((threadIdx.x & 63) == 0 && s < n) mask[s >> 6] = m;
}

// ---- device-side de-duplication of the candidates' DR strings (single-GPU merge fast path) ----
// Same 64-bit hash as TokenTable::hash (merge.cpp) so the host can reuse it.  Every distinct
// string gets one table slot; `first` keeps the smallest candidate index (= first occurrence in
// read order).  The host re-checks every (candidate, representative) pair with memcmp, so a hash
// collision between different strings is detected and only costs the fast path.
static __device__ uint64_t dr_hash64(const char *p, uint32_t n)
{
    uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)n * 0xD6E8FEB86659FD93ull);
    while (n >= 8) {
        uint64_t v = 0;
        for (int i = 0; i < 8; i++) v |= (uint64_t)(uint8_t)p[i] << (8 * i);
        h = (h ^ v) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; p += 8; n -= 8;
    }
    if (n) {
        uint64_t v = 0;
        for (uint32_t i = 0; i < n; i++) v |= (uint64_t)(uint8_t)p[i] << (8 * i);
        h = (h ^ v) * 0xC4CEB9FE1A85EC53ull; h ^= h >> 29;
    }
    return h ^ (h >> 31);
}

// found records -> compact hand-off blob + dense DR strings on the device + de-duplication insert
// (one thread per found record; see launch_gather_found in engine_internal.h)
// The insert goes through LDS first: most records carry one of a few popular strings, every resident thread meets the table
// while it is still empty, and returning atomics on one address retire one every 20-30 ns — 5.6 k compare-and-swaps on each
// popular slot were ~100 of this kernel's 125 us at 100 M reads.  A block of 1 024 records claims its strings in an LDS table
// (hash, smallest record index), then ONE thread per distinct string of the block goes to the global table.
#define GF_BLOCK 1024
#define GF_SLOTS 2048
__global__ __launch_bounds__(GF_BLOCK) void k_gather_found(const uint64_t *fidx, const uint32_t *d_nf, uint64_t n_max,
                                                            const SurvOut *out, const uint64_t *surv_idx, uint64_t read_base,
                                                            const char *dr_chars, uint32_t dr_stride, const uint32_t *ss_pool,
                                                            uint32_t ss_cap, uint32_t ss_elem, uint8_t *blob, uint16_t *g_dr_len, char *g_dr,
                                                            unsigned long long *dd_keys, uint32_t *dd_first, uint32_t dd_mask,
                                                            uint64_t *dd_hash, uint32_t *dd_slot, uint32_t *d_mismatch)
{
    __shared__ unsigned long long lkey[GF_SLOTS];
    __shared__ uint32_t lmin[GF_SLOTS], lslot[GF_SLOTS];
    const uint64_t k = blockIdx.x * (uint64_t)GF_BLOCK + threadIdx.x;
    uint64_t n = *d_nf;
    if (n > n_max) n = n_max;
    if (blockIdx.x * (uint64_t)GF_BLOCK >= n) return;    // (the launch is sized for the survivor bound)
    if (dd_keys) {
        for (uint32_t i = threadIdx.x; i < GF_SLOTS; i += GF_BLOCK) { lkey[i] = 0ull; lmin[i] = 0xFFFFFFFFu; }
        __syncthreads();
    }
    uint32_t ls = 0;
    if (k < n) {
        const P1Blob b = p1_blob_layout(n, ss_cap, ss_elem);
        const uint64_t s = fidx[k];
        const SurvOut o = out[s];
        reinterpret_cast<uint64_t *>(blob + b.read)[k] = read_base + surv_idx[s];
        reinterpret_cast<uint16_t *>(blob + b.replen)[k] = (uint16_t)o.repeat_len;
        (blob + b.nss)[k] = (uint8_t)o.n_ss;
        (blob + b.low)[k] = o.low_lexi;
        const uint32_t *ps = ss_pool + o.ss_off;
        if (ss_elem == 1 && (o.ss_off & 3u) == 0u) {         // ss_cap is a multiple of 4: whole words, and 16-byte loads (slot-mode pool)
            uint32_t *pd = reinterpret_cast<uint32_t *>(blob + b.ss + k * (uint64_t)ss_cap);
            const uint4 *p4 = reinterpret_cast<const uint4 *>(ps);
            for (uint32_t i = 0; i < ss_cap; i += 4) {
                const uint4 x = p4[i >> 2];
                const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
                uint32_t v = 0;
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) v |= ((i + q < o.n_ss) ? (xs[q] & 0xFFu) : 0u) << (8 * q);
                pd[i >> 2] = v;
            }
        } else if (ss_elem == 1) {
            uint32_t *pd = reinterpret_cast<uint32_t *>(blob + b.ss + k * (uint64_t)ss_cap);
            for (uint32_t i = 0; i < ss_cap; i += 4) {
                uint32_t v = 0;
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) v |= ((i + q < o.n_ss) ? (ps[i + q] & 0xFFu) : 0u) << (8 * q);
                pd[i >> 2] = v;
            }
        } else {
            uint32_t *pd = reinterpret_cast<uint32_t *>(blob + b.ss + k * (uint64_t)ss_cap * 2);
            for (uint32_t i = 0; i < ss_cap; i += 2) {
                const uint32_t lo = (i < o.n_ss) ? (ps[i] & 0xFFFFu) : 0u, hi = (i + 1 < o.n_ss) ? (ps[i + 1] & 0xFFFFu) : 0u;
                pd[i >> 1] = lo | (hi << 16);
            }
        }
        g_dr_len[k] = o.dr_len;
        // the string is copied 16 bytes at a time and hashed from the same registers (dr_hash64 over a zero-padded slot: a
        // partial last word IS the value its byte loop assembles; 36 byte loads per record were a third of this kernel)
        const uint4 *src = reinterpret_cast<const uint4 *>(dr_chars + s * (uint64_t)dr_stride);
        uint4 *dst = reinterpret_cast<uint4 *>(g_dr + k * (uint64_t)dr_stride);
        uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)o.dr_len * 0xD6E8FEB86659FD93ull);
        uint32_t rem = o.dr_len;
        for (uint32_t i = 0; i < dr_stride / 16; i++) {
            const uint4 v4 = src[i];
            dst[i] = v4;
            const uint64_t w2[2] = {(uint64_t)v4.x | ((uint64_t)v4.y << 32), (uint64_t)v4.z | ((uint64_t)v4.w << 32)};
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (rem >= 8) { h = (h ^ w2[q]) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; rem -= 8; }
                else if (rem) { h = (h ^ w2[q]) * 0xC4CEB9FE1A85EC53ull; h ^= h >> 29; rem = 0; }
            }
        }
        h ^= h >> 31;
        if (dd_keys) {
            // (the same 64-bit hash as TokenTable::hash, merge.cpp); 0 marks an empty slot
            dd_hash[k] = h;
            const unsigned long long key = h | 1ull;
            ls = (uint32_t)(h >> 40) & (GF_SLOTS - 1u);
            for (;;) {                                       // (at most 1 024 distinct keys in 2 048 slots: always ends)
                const unsigned long long old = atomicCAS(&lkey[ls], 0ull, key);
                if (old == 0ull || old == key) break;
                ls = (ls + 1u) & (GF_SLOTS - 1u);
            }
            atomicMin(&lmin[ls], (uint32_t)k);
        }
    }
    if (!dd_keys) return;
    __syncthreads();
    // The global table was cleared by the found-flag compaction.  It is sized for the DISTINCT strings the caller expects
    // (a learnt bound), not for the records: a probe sequence that outlasts kDdMaxProbes means the bound was too small.
    // Bit 2 of the mismatch word tells the host (which then de-duplicates itself and sizes the next call's table for the
    // records); the string keeps the occupied slot it stopped at, so that everything downstream stays in range.
    // Looking at a slot before the CAS / atomicMin pays at 100 M reads but costs two more round trips at 10 M: done for
    // launches sized for more than 2^20 records (the headline workload).
    const bool look = n_max > (1ull << 20);
    for (uint32_t i = threadIdx.x; i < GF_SLOTS; i += GF_BLOCK) {
        const unsigned long long key = lkey[i];
        if (key == 0ull) continue;
        uint32_t slot = (uint32_t)(key >> 17) & dd_mask;
        for (uint32_t probes = 0;; probes++) {
            unsigned long long old = look ? __hip_atomic_load(&dd_keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            if (old == 0ull) old = atomicCAS(&dd_keys[slot], 0ull, key);
            if (old == 0ull || old == key) break;
            if (probes >= kDdMaxProbes) { atomicOr(d_mismatch, 2u); break; }
            slot = (slot + 1) & dd_mask;
        }
        const uint32_t kmin = lmin[i];
        if (!look || __hip_atomic_load(&dd_first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > kmin) atomicMin(&dd_first[slot], kmin);
        lslot[i] = slot;
    }
    __syncthreads();
    if (k < n) dd_slot[k] = lslot[ls];
}

// k_found_mask + compaction in one pass (decoupled look-back): survivor slot s -> rank among the found records ->
// fidx[rank] = s.  Also clears the de-duplication table of the next stage.  (The gather itself stays a dense kernel:
// with one found record in six slots a fused body would run at a sixth of the lanes.)  Tiles of 16 384 slots (16 per
// thread); the launch is sized for the survivor BOUND, tiles past the device-side count leave at once.
static constexpr uint32_t kFcPerThread = 16, kFcTile = 1024u * kFcPerThread;
// Wave w of the block takes slots [w * 1024, (w + 1) * 1024) of the tile, 64 consecutive slots per step (one per lane: the
// loads of a step cover one contiguous 1 280-byte run); a step's found flags are one ballot.
__global__ __launch_bounds__(1024) void k_found_compact(const SurvOut *out, const uint32_t *d_n, uint64_t n_max, uint32_t *d_err,
                                                         unsigned long long *dd_keys, uint32_t *dd_first, uint32_t dd_size,
                                                         uint64_t *fidx, uint32_t *d_nf, Lookback lb)
{
    uint64_t n = *d_n;                                   // slots past the device-side count were never written
    if (n > n_max) n = n_max;
    const uint32_t n_act = n ? (uint32_t)((n + kFcTile - 1) / kFcTile) : 1u;
    if (blockIdx.x >= n_act) return;
    const uint32_t tile = lb_tile_id(lb, n_act);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t s0 = (uint64_t)tile * kFcTile + (uint64_t)wv * 1024u;
    for (uint64_t i = (uint64_t)tile * 1024u + threadIdx.x; i < dd_size; i += (uint64_t)n_act * 1024u) { dd_keys[i] = 0ull; dd_first[i] = 0xFFFFFFFFu; }
    uint32_t err = 0, cnt = 0;
    uint64_t fm[kFcPerThread];
#pragma unroll
    for (uint32_t e = 0; e < kFcPerThread; e++) {
        const uint64_t sl = s0 + e * 64u + (uint32_t)lane;
        bool f = false;
        if (sl < n) { f = out[sl].found != 0; err = max(err, (uint32_t)out[sl].err); }
        fm[e] = __ballot(f);
        cnt += (uint32_t)__popcll(fm[e]);                // (wave-uniform)
    }
    if (err) atomicMax(d_err, err);
    // ranks: the wave's base from a scan over the 16 wave totals, then step by step
    __shared__ uint32_t wtot[16];
    if (lane == 0) wtot[wv] = cnt;
    __syncthreads();
    uint32_t wbase = 0, all = 0;
#pragma unroll
    for (int q = 0; q < 16; q++) { const uint32_t t = wtot[q]; if (q < wv) wbase += t; all += t; }
    const uint32_t excl = lb_exclusive_prefix(lb, tile, all);
    if (tile == n_act - 1 && threadIdx.x == 0) *d_nf = excl + all;
    uint64_t k = (uint64_t)excl + wbase;
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t e = 0; e < kFcPerThread; e++) {
        if ((fm[e] >> lane) & 1ull) fidx[k + (uint32_t)__popcll(fm[e] & lt)] = s0 + e * 64u + (uint32_t)lane;
        k += (uint32_t)__popcll(fm[e]);
    }
}
hipError_t launch_found_compact(const SurvOut *out, const uint32_t *d_n, uint64_t n_max, uint32_t *d_err, unsigned long long *dd_keys,
                                uint32_t *dd_first, uint32_t dd_size, uint64_t *fidx, uint32_t *d_nf, const Lookback &lb, hipStream_t st)
{
    if (n_max == 0) return hipSuccess;
    const uint32_t n_tiles = (uint32_t)((n_max + kFcTile - 1) / kFcTile);
    CRASS_LAUNCH(k_found_compact, dim3(n_tiles), dim3(1024), 0, st, out, d_n, n_max, d_err, dd_keys, dd_first, dd_keys ? dd_size : 0u,
                       fidx, d_nf, lb);
    return hipGetLastError();
}

// ---- host-loop sink: select + gather of the found records (engine_internal.h) ----
__global__ __launch_bounds__(256) void k_select_found(const SurvOut *out, uint64_t n, uint64_t *mask, uint32_t *d_err)
{
    const uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    bool f = false;
    if (s < n) {
        const SurvOut o = out[s];
        f = o.found != 0 && o.err == 0;
        if (o.err && o.err != 5) atomicMax(d_err, o.err == 1 ? 2u : 1u);
    }
    const uint64_t m = __ballot(f);
    if ((threadIdx.x & 63) == 0 && s < n) mask[s >> 6] = m;
}
__global__ __launch_bounds__(256) void k_gather_sparse(const uint64_t *fidx, const uint32_t *d_nf, uint64_t n_max, const SurvOut *out, const char *dr_chars,
                                                        uint32_t dr_stride, const uint32_t *ss_pool, SurvOut *g_out, uint64_t *g_slot, char *g_dr,
                                                        uint32_t *g_ss, uint32_t g_ss_cap, uint32_t *d_ss_total, uint16_t *g_dr_len, int ss16)
{
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint64_t n = *d_nf;
    if (n > n_max) n = n_max;
    SurvOut o; o.found = 0; o.n_ss = 0; o.repeat_len = 0; o.ss_off = 0; o.dr_len = 0; o.low_lexi = 0; o.err = 0;
    uint64_t s = 0;
    if (k < n) { s = fidx[k]; o = out[s]; }
    const uint32_t off = block_reserve<256>(k < n ? o.n_ss : 0u, d_ss_total);      // (every thread of the block)
    if (k >= n) return;
    // (ss16: every position of the set fits 16 bits — the packed pool then travels in half the bytes: 50 k records with 80
    // start/stops each are 16 MB of a long-read step's 20 MB of copies)
    if ((uint64_t)off + o.n_ss <= g_ss_cap) {
        if (ss16) { uint16_t *g16 = reinterpret_cast<uint16_t *>(g_ss); for (uint32_t i = 0; i < o.n_ss; i++) g16[off + i] = (uint16_t)ss_pool[o.ss_off + i]; }
        else for (uint32_t i = 0; i < o.n_ss; i++) g_ss[off + i] = ss_pool[o.ss_off + i];
    }
    o.ss_off = off;
    g_out[k] = o;
    g_slot[k] = s;
    if (g_dr_len) g_dr_len[k] = o.dr_len;               // (dense lengths: the de-duplication that may follow on the device)
    const char *src = dr_chars + s * (uint64_t)dr_stride;
    char *dst = g_dr + k * (uint64_t)dr_stride;
    for (uint32_t i = 0; i < dr_stride; i++) dst[i] = src[i];
}
hipError_t launch_select_found(const SurvOut *out, uint64_t n, uint64_t *mask, uint32_t *d_err, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    CRASS_LAUNCH(k_select_found, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, n, mask, d_err);
    return hipGetLastError();
}
hipError_t launch_gather_sparse(const uint64_t *fidx, const uint32_t *d_nf, uint64_t n_max, const SurvOut *out, const char *dr_chars, uint32_t dr_stride,
                                const uint32_t *ss_pool, SurvOut *g_out, uint64_t *g_slot, char *g_dr, uint32_t *g_ss, uint32_t g_ss_cap,
                                uint32_t *d_ss_total, hipStream_t st, uint16_t *g_dr_len, int ss16)
{
    if (n_max == 0) return hipSuccess;
    CRASS_LAUNCH(k_gather_sparse, dim3((unsigned)((n_max + 255) / 256)), dim3(256), 0, st, fidx, d_nf, n_max, out, dr_chars, dr_stride, ss_pool,
                       g_out, g_slot, g_dr, g_ss, g_ss_cap, d_ss_total, g_dr_len, ss16);
    return hipGetLastError();
}

hipError_t launch_found_mask(const SurvOut *out, const uint32_t *d_n, uint64_t n, uint64_t *mask, uint32_t *d_err, hipStream_t st,
                             unsigned long long *dd_keys, uint32_t *dd_first, uint32_t dd_size)
{
    if (n == 0) return hipSuccess;
    CRASS_LAUNCH(k_found_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, d_n, n, mask, d_err, dd_keys, dd_first, dd_keys ? dd_size : 0u);
    return hipGetLastError();
}

hipError_t launch_gather_found(const uint64_t *fidx, const uint32_t *d_nf, uint64_t n_max, const SurvOut *out,
                               const uint64_t *surv_idx, uint64_t read_base, const char *dr_chars, uint32_t dr_stride,
                               const uint32_t *ss_pool, uint32_t ss_cap, uint32_t ss_elem, uint8_t *h_blob,
                               uint16_t *g_dr_len, char *g_dr, hipStream_t st,
                               unsigned long long *dd_keys, uint32_t *dd_first, uint32_t dd_size, uint64_t *dd_hash, uint32_t *dd_slot,
                               uint32_t *d_mismatch)
{
    if (n_max == 0) return hipSuccess;
    if ((ss_cap & 3u) || (ss_elem != 1 && ss_elem != 2)) return hipErrorInvalidValue;
    CRASS_LAUNCH(k_gather_found, dim3((unsigned)((n_max + GF_BLOCK - 1) / GF_BLOCK)), dim3(GF_BLOCK), 0, st, fidx, d_nf, n_max, out, surv_idx,
                       read_base, dr_chars, dr_stride, ss_pool, ss_cap, ss_elem, h_blob, g_dr_len, g_dr,
                       dd_keys, dd_first, dd_keys ? dd_size - 1 : 0u, dd_hash, dd_slot, d_mismatch);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_dr_dedupe_clear(unsigned long long *keys, uint32_t *first, uint32_t table_size)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < table_size; i += gridDim.x * blockDim.x) { keys[i] = 0ull; first[i] = 0xFFFFFFFFu; }
}

__global__ __launch_bounds__(256) void k_dr_dedupe_insert(const char *dr, const uint16_t *dr_len, uint32_t stride, const uint32_t *d_n,
                                                           uint32_t n_max, unsigned long long *keys, uint32_t *first, uint32_t mask,
                                                           uint64_t *hash_out, uint32_t *slot_out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = min(*d_n, n_max);
    if (k >= n) return;
    const uint64_t h = dr_hash64(dr + (uint64_t)k * stride, dr_len[k]);
    hash_out[k] = h;
    const unsigned long long key = h | 1ull;                 // 0 marks an empty slot
    uint32_t slot = (uint32_t)(h >> 17) & mask;
    for (;;) {
        const unsigned long long old = atomicCAS(&keys[slot], 0ull, key);
        if (old == 0ull || old == key) break;
        slot = (slot + 1) & mask;
    }
    atomicMin(&first[slot], k);
    slot_out[k] = slot;
}

// the candidate count lives on the device (*d_n, at most n_max): no host round trip before this launch
hipError_t launch_dr_dedupe(const char *dr, const uint16_t *dr_len, uint32_t stride, const uint32_t *d_n, uint32_t n, unsigned long long *keys,
                            uint32_t *first, uint32_t table_size, uint64_t *hash_out, uint32_t *slot_tmp, uint32_t *rep, hipStream_t st,
                            bool table_cleared)
{
    if (n == 0) return hipSuccess;
    if (!table_cleared) CRASS_LAUNCH(k_dr_dedupe_clear, dim3((unsigned)std::min<uint32_t>((table_size + 255) / 256, 2048u)), dim3(256), 0, st, keys, first, table_size);
    const unsigned nb = (n + 255) / 256;
    CRASS_LAUNCH(k_dr_dedupe_insert, dim3(nb), dim3(256), 0, st, dr, dr_len, stride, d_n, n, keys, first, table_size - 1, hash_out, slot_tmp);
    (void)rep;                                  // rep[] = first occurrence of every candidate: written by k_dx_flag
    return hipGetLastError();
}

// ---- device-side token ranks: distinct strings in first-occurrence order ----
// bit k of `mask` = candidate k is the first occurrence of its string; every other candidate is compared
// byte for byte with its representative, so a 64-bit hash collision between different strings is
// DETECTED (flag) and the host then takes its plain path.
__global__ __launch_bounds__(256) void k_dx_flag(const char *dr, const uint16_t *dr_len, uint32_t stride, const uint32_t *d_n, uint32_t n_max,
                                                  const uint32_t *slot_of, const uint32_t *first, uint32_t *rep, uint64_t *mask, uint32_t *d_mismatch)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = min(*d_n, n_max);
    bool is_rep = false;
    if (k < n) {
        const uint32_t f = first[slot_of[k]];               // (was k_dr_dedupe_rep: one launch less)
        rep[k] = f;
        is_rep = (f == k);
        if (!is_rep) {
            bool same = f < k && dr_len[f] == dr_len[k];
            if (same) {
                const uint4 *a = reinterpret_cast<const uint4 *>(dr + (uint64_t)k * stride);
                const uint4 *b = reinterpret_cast<const uint4 *>(dr + (uint64_t)f * stride);
                for (uint32_t i = 0; i < stride / 16; i++) {          // slots are zero padded: whole-slot compare
                    const uint4 x = a[i], y = b[i];
                    same = same && x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
                }
            }
            if (!same) atomicOr(d_mismatch, 1u);
        }
    }
    const uint64_t m = __ballot(is_rep);
    if ((threadIdx.x & 63) == 0 && k < n_max) mask[k >> 6] = m;       // words past the count are zero
}

// dmap[k] = rank of k's representative among the first occurrences (token = rank + 2 on one GPU)
__global__ __launch_bounds__(256) void k_dx_assign(const uint32_t *rep, const uint32_t *d_n, uint32_t n_max, const uint64_t *mask,
                                                    const uint32_t *word_prefix, const uint32_t *block_sums, uint32_t *dmap)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= min(*d_n, n_max)) return;
    const uint32_t f = rep[k], w = f >> 6;
    dmap[k] = block_sums[w >> 8] + word_prefix[w] + (uint32_t)__popcll(mask[w] & ((1ull << (f & 63)) - 1ull));
}

__global__ __launch_bounds__(256) void k_dx_gather(const uint64_t *dx_idx, const uint32_t *d_nd, uint32_t n_max, const char *dr,
                                                    const uint16_t *dr_len, const uint64_t *hash, uint32_t stride, char *out_chars,
                                                    uint16_t *out_len, uint64_t *out_hash, char *dev_chars, uint16_t *dev_len,
                                                    const uint32_t *cnt_src, uint32_t *cnt_dst, uint32_t n_cnt)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_cnt) cnt_dst[j] = cnt_src[j];             // the stage's counters, straight into pinned host memory
    uint32_t nd = *d_nd;
    if (nd > n_max) nd = n_max;
    if (j >= nd) return;
    const uint64_t k = dx_idx[j];
    const uint4 *src = reinterpret_cast<const uint4 *>(dr + k * stride);
    uint4 *dst = reinterpret_cast<uint4 *>(out_chars + (uint64_t)j * stride);
    uint4 *dst2 = reinterpret_cast<uint4 *>(dev_chars + (uint64_t)j * stride);      // device copy for the device merge
    // (out_*: pinned host memory, or nullptr when nobody on the host reads the list — the device merge exports its own view)
    for (uint32_t i = 0; i < stride / 16; i++) { const uint4 v = src[i]; if (out_chars) dst[i] = v; if (dev_chars) dst2[i] = v; }
    const uint16_t l = dr_len[k];
    if (out_len) out_len[j] = l;
    if (dev_len) dev_len[j] = l;
    if (out_hash) out_hash[j] = hash[k];
}

// k_dx_flag + compaction in one pass (decoupled look-back over tiles of 1024 candidates, one per thread: the body is a
// chain of dependent loads, so it wants many blocks rather than fat ones): candidate k is a first occurrence iff
// first[slot_of[k]] == k; dx_idx[rank] = k, and the representative's rank is left in slot_of[k] (every thread only
// ever reads its OWN slot_of entry here, so overwriting it is safe) for the assign kernel that follows.
__global__ __launch_bounds__(1024) void k_dx_flag_compact(const char *dr, const uint16_t *dr_len, uint32_t stride, const uint32_t *d_n, uint32_t n_max,
                                                           uint32_t *slot_of, const uint32_t *first, uint32_t *rep, uint64_t *dx_idx, uint32_t *d_nd,
                                                           uint32_t *d_mismatch, Lookback lb)
{
    const uint32_t n = min(*d_n, n_max);
    const uint32_t n_tiles = n ? (n + 1023u) / 1024u : 1u;          // (the launch is sized for a bound: the tiles past the count leave at once)
    if (blockIdx.x >= n_tiles) return;
    const uint32_t tile = lb_tile_id(lb, n_tiles);
    const uint32_t k = tile * 1024u + threadIdx.x;
    bool is_rep = false;
    if (k < n) {
        const uint32_t f = first[slot_of[k]];
        rep[k] = f;
        is_rep = (f == k);
        if (!is_rep) {
            bool same = f < k && dr_len[f] == dr_len[k];
            if (same) {
                const uint4 *a = reinterpret_cast<const uint4 *>(dr + (uint64_t)k * stride);
                const uint4 *b = reinterpret_cast<const uint4 *>(dr + (uint64_t)f * stride);
                for (uint32_t i = 0; i < stride / 16; i++) {          // slots are zero padded: whole-slot compare
                    const uint4 x = a[i], y = b[i];
                    same = same && x.x == y.x && x.y == y.y && x.z == y.z && x.w == y.w;
                }
            }
            if (!same) atomicOr(d_mismatch, 1u);
        }
    }
    uint32_t all;
    const uint32_t in_tile = block_scan_t<1024>(is_rep ? 1u : 0u, &all);
    const uint32_t excl = lb_exclusive_prefix(lb, tile, all);
    if (tile == n_tiles - 1 && threadIdx.x == 0) *d_nd = excl + all;
    if (is_rep) { const uint32_t q = excl + in_tile; dx_idx[q] = k; slot_of[k] = q; }
}

// dense: every candidate's rank (dmap = rank of its representative) and, for the first nd threads, the distinct string's slot
__global__ __launch_bounds__(256) void k_dx_assign_gather(const uint32_t *rep, const uint32_t *d_n, uint32_t n_max, const uint32_t *rank_of,
                                                           uint32_t *dmap, const uint64_t *dx_idx, const uint32_t *d_nd, const char *dr,
                                                           const uint16_t *dr_len, const uint64_t *hash, uint32_t stride, char *out_chars,
                                                           uint16_t *out_len, uint64_t *out_hash, char *dev_chars, uint16_t *dev_len,
                                                           const uint32_t *cnt_src, uint32_t *cnt_dst, uint32_t n_cnt)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_cnt) cnt_dst[j] = cnt_src[j];             // the stage's counters, straight into pinned host memory
    if (j < min(*d_n, n_max)) dmap[j] = rank_of[rep[j]];
    uint32_t nd = *d_nd;
    if (nd > n_max) nd = n_max;
    if (j >= nd) return;
    const uint64_t k = dx_idx[j];
    const uint4 *src = reinterpret_cast<const uint4 *>(dr + k * stride);
    uint4 *dst = reinterpret_cast<uint4 *>(out_chars + (uint64_t)j * stride);
    uint4 *dst2 = reinterpret_cast<uint4 *>(dev_chars + (uint64_t)j * stride);      // device copy for the device merge
    // (out_*: pinned host memory, or nullptr when nobody on the host reads the list — the device merge exports its own view)
    for (uint32_t i = 0; i < stride / 16; i++) { const uint4 v = src[i]; if (out_chars) dst[i] = v; if (dev_chars) dst2[i] = v; }
    const uint16_t l = dr_len[k];
    if (out_len) out_len[j] = l;
    if (dev_len) dev_len[j] = l;
    if (out_hash) out_hash[j] = hash[k];
}

// needs stride % 16 == 0; mask / word_prefix / block_sums / dx_idx are scratch of >= n bits / words.  The candidate
// count is *d_n (<= n).  dmap / out_* may be pinned host memory: the kernels then write the merge's inputs
// straight into it (a few hundred KB; no copy calls on the critical path).
hipError_t launch_dx_tokens(const char *dr, const uint16_t *dr_len, const uint64_t *hash, uint32_t stride, const uint32_t *d_n, uint32_t n, uint32_t *rep,
                            uint32_t *slot_of, const uint32_t *first,
                            uint64_t *mask, uint32_t *word_prefix, uint32_t *block_sums, uint64_t *dx_idx, uint32_t *d_nd,
                            uint32_t *d_mismatch, uint32_t *dmap, char *out_chars, uint16_t *out_len, uint64_t *out_hash,
                            char *dev_chars, uint16_t *dev_len, hipStream_t st, const uint32_t *cnt_src, uint32_t *cnt_dst, uint32_t n_cnt,
                            const Lookback *lb)
{
    if (n == 0) return hipSuccess;
    const unsigned nb = (n + 255) / 256;
    if (lb) {           // two launches: flags + single-pass compaction (element-wise look-back), dense assign + gather
        const uint32_t n_tiles = (n + 1023u) / 1024u;                               // (the caller reserved that many tickets)
        CRASS_LAUNCH(k_dx_flag_compact, dim3(n_tiles), dim3(1024), 0, st, dr, dr_len, stride, d_n, n, slot_of, first, rep, dx_idx, d_nd, d_mismatch,
                           *lb);
        CRASS_LAUNCH(k_dx_assign_gather, dim3(nb), dim3(256), 0, st, rep, d_n, n, (const uint32_t *)slot_of, dmap, dx_idx, d_nd, dr, dr_len,
                           hash, stride, out_chars, out_len, out_hash, dev_chars, dev_len, cnt_src, cnt_dst, cnt_dst ? n_cnt : 0u);
        return hipGetLastError();
    }
    CRASS_LAUNCH(k_dx_flag, dim3(nb), dim3(256), 0, st, dr, dr_len, stride, d_n, n, slot_of, first, rep, mask, d_mismatch);
    hipError_t e = launch_compact(mask, (n + 63) / 64, n, word_prefix, block_sums, dx_idx, n, d_nd, st);
    if (e != hipSuccess) return e;
    CRASS_LAUNCH(k_dx_assign, dim3(nb), dim3(256), 0, st, rep, d_n, n, mask, word_prefix, block_sums, dmap);
    CRASS_LAUNCH(k_dx_gather, dim3(nb), dim3(256), 0, st, dx_idx, d_nd, n, dr, dr_len, hash, stride, out_chars, out_len, out_hash, dev_chars, dev_len,
                       cnt_src, cnt_dst, cnt_dst ? n_cnt : 0u);
    return hipGetLastError();
}

// ---- pass-2 sink on the device: drop the slots without a match, pack the rest (read order) ----
__global__ __launch_bounds__(256) void k_recruit_valid_mask(const RecruitOut *rec, const uint32_t *d_n, uint64_t n_max, uint64_t *mask)
{
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint64_t n = *d_n;
    if (n > n_max) n = n_max;
    const bool v = k < n && rec[k].dr_len != 0;
    const uint64_t m = __ballot(v);
    if ((threadIdx.x & 63) == 0 && k < n_max) mask[k >> 6] = m;
}
__global__ __launch_bounds__(256) void k_pack_p2_blob(const RecruitOut *rec, const uint64_t *hit_idx, uint64_t read_base, const uint64_t *vidx,
                                                       const uint32_t *d_nv, uint64_t cap, uint8_t *blob, const uint32_t *d_n_hits, uint32_t *h_n_hits,
                                                       uint32_t narrow)
{
    const uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint64_t nv = *d_nv;
    if (nv > cap) nv = cap;
    if (q == 0) {
        reinterpret_cast<uint64_t *>(blob)[0] = nv; reinterpret_cast<uint64_t *>(blob)[1] = cap;
        if (h_n_hits) *h_n_hits = *d_n_hits;            // the flagged-read count the host checks its bound against
    }
    if (q >= nv) return;
    const P2Blob b = p2_blob_layout(cap, narrow);
    const uint64_t k = vidx[q];
    const RecruitOut o = rec[k];
    if (narrow == 2) {
        reinterpret_cast<uint32_t *>(blob + b.token)[q] = o.token | ((uint32_t)(o.low_lexi != 0) << 31);
        reinterpret_cast<uint32_t *>(blob + b.read)[q] = (uint32_t)hit_idx[k];
        (blob + b.start)[q] = (uint8_t)o.start;
        return;
    }
    reinterpret_cast<uint32_t *>(blob + b.token)[q] = o.token;
    if (narrow) {
        reinterpret_cast<uint32_t *>(blob + b.read)[q] = (uint32_t)hit_idx[k];          // (local index: the host adds the base)
        (blob + b.start)[q] = (uint8_t)o.start;
        (blob + b.end)[q] = (uint8_t)o.end;
    } else {
        reinterpret_cast<uint64_t *>(blob + b.read)[q] = read_base + hit_idx[k];
        reinterpret_cast<uint16_t *>(blob + b.start)[q] = (uint16_t)o.start;
        reinterpret_cast<uint16_t *>(blob + b.end)[q] = (uint16_t)o.end;
    }
    (blob + b.dr_len)[q] = (uint8_t)o.dr_len;
    (blob + b.low)[q] = o.low_lexi;
}
// k_recruit_valid_mask + compaction in one pass (decoupled look-back): vidx[rank] = slot of the rank-th valid hit
__global__ __launch_bounds__(1024) void k_valid_compact(const RecruitOut *rec, const uint32_t *d_n_hits, uint64_t cap, uint64_t *vidx, uint32_t *d_nv,
                                                         Lookback lb)
{
    uint64_t n = *d_n_hits;
    if (n > cap) n = cap;
    const uint32_t n_tiles = n ? (uint32_t)((n + kLbElemsPerTile - 1) / kLbElemsPerTile) : 1u;      // (sized for a bound: the tiles past the count leave at once)
    if (blockIdx.x >= n_tiles) return;
    const uint32_t tile = lb_tile_id(lb, n_tiles);
    const uint64_t k0 = (uint64_t)tile * kLbElemsPerTile + 4u * threadIdx.x;
    uint32_t fm = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) if (k0 + e < n && rec[k0 + e].dr_len != 0) fm |= 1u << e;
    uint32_t upto;
    uint64_t q = lb_rank4(lb, tile, (uint32_t)__popc(fm), &upto);
    if (tile == n_tiles - 1 && threadIdx.x == 0) *d_nv = upto;
#pragma unroll
    for (int e = 0; e < 4; e++) if (fm & (1u << e)) vidx[q++] = k0 + e;
}

hipError_t launch_pack_p2_blob(const RecruitOut *rec, const uint64_t *hit_idx, uint64_t read_base,
                               const uint32_t *d_n_hits, uint64_t n_hits_max, uint64_t *mask, uint32_t *word_prefix, uint32_t *block_sums,
                               uint64_t *vidx, uint32_t *d_nv, uint8_t *blob, hipStream_t st, uint32_t *h_n_hits, const Lookback *lb, uint32_t narrow)
{
    if (n_hits_max == 0) return hipSuccess;
    const unsigned nb = (unsigned)((n_hits_max + 255) / 256);
    if (lb) {           // (the caller reserved nb tiles)
        const unsigned nt = (unsigned)((n_hits_max + kLbElemsPerTile - 1) / kLbElemsPerTile);
        CRASS_LAUNCH(k_valid_compact, dim3(nt), dim3(1024), 0, st, rec, d_n_hits, n_hits_max, vidx, d_nv, *lb);
        CRASS_LAUNCH(k_pack_p2_blob, dim3(nb), dim3(256), 0, st, rec, hit_idx, read_base, vidx, d_nv, n_hits_max, blob, d_n_hits, h_n_hits, narrow);
        return hipGetLastError();
    }
    CRASS_LAUNCH(k_recruit_valid_mask, dim3(nb), dim3(256), 0, st, rec, d_n_hits, n_hits_max, mask);
    hipError_t e = launch_compact(mask, (n_hits_max + 63) / 64, n_hits_max, word_prefix, block_sums, vidx, n_hits_max, d_nv, st);
    if (e != hipSuccess) return e;
    CRASS_LAUNCH(k_pack_p2_blob, dim3(nb), dim3(256), 0, st, rec, hit_idx, read_base, vidx, d_nv, n_hits_max, blob, d_n_hits, h_n_hits, narrow);
    return hipGetLastError();
}

} // namespace crass
