// gunzip.hip — one plain gzip member inflated on the device chunk by chunk: the rule is gunzip_core.h's, statement for statement
// what the host runs (gunzip.cpp); this file only says how waves go through it.  Five launches, none waits for another's waves:
//   k_gz_find     a wave per chunk, grid-stride.  The 64 lanes test 64 consecutive bit positions at a time in registers
//                 (gz_survives: BFINAL / BTYPE, HLIT, HDIST, the code-length code's Kraft sum); a ballot gives the survivors,
//                 which the whole wave takes in ascending position through the header parse and the two trial block decodes
//   k_gz_count    a wave per chunk: the blocks from its start to the next chunk's start it runs into, storing nothing
//   k_gz_decode   a wave per chain element: the same bits again, as 16-bit symbols at the element's exact place in HBM
//   k_gz_windows  ONE workgroup walks the chain in order, 32 768 entries per element
//   k_gz_narrow   a workgroup per chain element: symbols to bytes through the element's window, aligned 16-byte stores with byte
//                 stores only in the first and last partial vector (as k_fetch_text), then the element's CRC-32 in 256 slices
// Members mode (a file of several members, gunzip_core.h) runs the same five through k_gz_find_members, k_gz_count_members,
// k_gz_decode_members and k_gz_narrow_members (the same bodies with the rule's MEM parameter on; narrow then leaves the CRC to)
//   k_gz_member_crc  a wave per piece of text (cut at member boundaries and every 64 KB inside a member): 64 lane slices, as
//                    k_gz_narrow's 256
// A range of the file (a rank of a group, crass_hip_group_inflate_gzip): the same kernels over the chunks [k0, k1) and the chain
// elements [e0, e0 + n_chain) of a job that holds only the bytes d[in_lo, in_hi) its runs may read (GzJob; a whole file is the
// full range), and in place of k_gz_windows, which needs the window in front of the range's first element,
//   k_gz_windows_sym     ONE workgroup walks the RANGE's elements from the identity: windows of bytes and references into the
//                        unknown entry window (gz_window_entry_sym)
//                        (k_gz_windows_sym_members: dead entries read 0, gunzip_core.h)
//   k_gz_window_resolve  a workgroup per element, once the host has composed the ranges' entry windows: symbolic to bytes
// As in inflate.hip: symbol decoding is serial, all 64 lanes run it with the same values; tables (BzTables, 7 KB per wave) are in
// LDS, the text in HBM; what a lane wrote is read by lanes of the SAME wave only, so io.sync() is a wavefront-scope fence plus a
// wave barrier (see inflate.hip for the memory model's wording); no workgroup barrier inside the serial decode.
// Scratch is the engine's: 2 bytes per text byte (sym) plus 32 KB per chain element (win), taken from dev_alloc and given back
// before the call returns.
// Bounds: input is read inside d[in_lo, in_hi) only, a whole file's d[0, dn) (at() cuts a run's input to it, in() and gz_survives
// check the index); find writes start[k0, k1), count link / text_len / end_bit / reason [k0, k1); k_gz_windows_sym writes
// wsym[32768 i, 32768 (i + 1)) for i in [1, n_win]; k_gz_window_resolve writes win[32768 i, 32768 (i + 1)) for i in
// [1, n_win]; a decode wave writes sym[off[i], off[i+1])
// only (put() checks) and in members mode ends[slot[i] - slot[0], slot[i+1] - slot[0]) (end() checks); k_gz_member_crc reads out[piece[q], piece[q+1])
// and writes crc_piece[q]; k_gz_windows writes win[32768 i, 32768 (i + 1)); k_gz_narrow writes out[off[i], off[i+1]).
#include "gunzip_launch.h"
#include "engine_internal.h"
#include "devmem.h"

namespace crass {

static constexpr int kGzWaves = 4;                        // waves per workgroup in find / count / decode
static constexpr int kGzNarrowThreads = 256, kGzWindowThreads = 1024;

struct GzWaveIO {
    const uint8_t *d; uint64_t dn; const uint8_t *src; uint32_t n_in; uint16_t *sym; uint64_t cap; uint32_t lane;
    GzEnd *ends = nullptr; uint32_t ends_cap = 0;         // (members mode)
    uint64_t lo = 0, hi = 0;                              // the staged bytes d[lo, hi), hi <= dn (a whole file: [0, dn))
    // (a run's input is cut to what is staged: a job stages what its runs may read, so nothing is cut that a whole-file run reads)
    __device__ __forceinline__ void at(uint64_t b0, uint32_t n)
    {
        src = d + b0;
        n_in = b0 < lo || b0 >= hi ? 0u : (uint32_t)(hi - b0 < n ? hi - b0 : n);
    }
    __device__ __forceinline__ uint32_t in(uint32_t i) const { return i < n_in ? (uint32_t)src[i] : 0u; }
    __device__ __forceinline__ void put(uint64_t p, uint32_t s) { if (p < cap) sym[p] = (uint16_t)s; }
    __device__ __forceinline__ uint32_t get(uint64_t p) const { return p < cap ? (uint32_t)sym[p] : 0u; }
    template <class F> __device__ __forceinline__ void par(uint32_t n, F f) { for (uint32_t i = lane; i < n; i += 64u) f(i); }
    __device__ __forceinline__ bool lead() const { return lane == 0; }
    __device__ __forceinline__ void sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // lane l answers for position base + l
    __device__ __forceinline__ uint64_t survivors(uint64_t base, uint64_t top, uint64_t limit) const
    {
        return (uint64_t)__ballot(gz_survives(d, hi, base + lane, top, limit, lo) ? 1 : 0);
    }
    // (members mode only; clipped to what is staged as survivors is)
    __device__ __forceinline__ uint64_t header_survivors(uint64_t base, uint64_t top, uint64_t limit) const
    {
        return (uint64_t)__ballot(gz_survives_header(d, hi, base + lane, top, limit, lo) ? 1 : 0);
    }
    // the file's last 8 bytes, where the job staged them (a whole file; of a group the ranks whose find runs see the region's end)
    bool has_tail = false;
    __device__ __forceinline__ uint32_t tail(uint32_t i) const { return has_tail && i < 8u ? (uint32_t)d[dn + i] : 0u; }
    __device__ __forceinline__ void end(uint32_t e, const GzEnd &r) { if (e < ends_cap) ends[e] = r; }
};

template <bool MEM> __device__ __forceinline__ void gz_find_waves(const GzJob &J, BzTables *tabs)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    BzTables &T = tabs[wv];
    GzWaveIO io{J.d, J.G.dn, J.d, 0, nullptr, 0, lane};
    io.lo = J.in_lo; io.hi = J.in_hi; io.has_tail = J.in_tail != 0;
    bz_prepare(io, T);
    const uint64_t n_waves = (uint64_t)gridDim.x * kGzWaves;
    for (uint64_t k = J.k0 + (uint64_t)blockIdx.x * kGzWaves + wv; k < J.k1; k += n_waves) {
        const uint64_t s = k ? gz_find<MEM>(io, T, J.G, k) : 0;
        if (lane == 0) J.start[k] = s;
        io.sync();
    }
}
__global__ __launch_bounds__(64 * kGzWaves) void k_gz_find(GzJob J)
{
    __shared__ BzTables tabs[kGzWaves];
    gz_find_waves<false>(J, tabs);
}
__global__ __launch_bounds__(64 * kGzWaves) void k_gz_find_members(GzJob J)
{
    __shared__ BzTables tabs[kGzWaves];
    gz_find_waves<true>(J, tabs);
}

template <bool MEM> __device__ __forceinline__ void gz_count_waves(const GzJob &J, BzTables *tabs)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    BzTables &T = tabs[wv];
    GzWaveIO io{J.d, J.G.dn, J.d, 0, nullptr, 0, lane};
    io.lo = J.in_lo; io.hi = J.in_hi; io.has_tail = J.in_tail != 0;
    bz_prepare(io, T);
    const uint64_t n_waves = (uint64_t)gridDim.x * kGzWaves;
    for (uint64_t k = J.k0 + (uint64_t)blockIdx.x * kGzWaves + wv; k < J.k1; k += n_waves) {
        const uint64_t s = J.start[k];
        GzRun R{BZ_OK, GZ_LINK_NONE, 0, 0, 0, 0};
        if (s != kGzNoStart) R = gz_run<GZ_COUNT, MEM>(io, T, J.G, k, s, J.start, 0);
        if (lane == 0) { J.link[k] = R.link; J.text_len[k] = R.text; J.end_bit[k] = R.end_bit; J.reason[k] = R.reason; }
        if (MEM && lane == 0) { J.n_ends[k] = R.n_ends; J.last_end[k] = R.last_end; }
        io.sync();
    }
}
__global__ __launch_bounds__(64 * kGzWaves) void k_gz_count(GzJob J)
{
    __shared__ BzTables tabs[kGzWaves];
    gz_count_waves<false>(J, tabs);
}
__global__ __launch_bounds__(64 * kGzWaves) void k_gz_count_members(GzJob J)
{
    __shared__ BzTables tabs[kGzWaves];
    gz_count_waves<true>(J, tabs);
}

template <bool MEM> __device__ __forceinline__ void gz_decode_waves(const GzJob &J, BzTables *tabs)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    BzTables &T = tabs[wv];
    GzWaveIO io{J.d, J.G.dn, J.d, 0, nullptr, 0, lane};
    io.lo = J.in_lo; io.hi = J.in_hi; io.has_tail = J.in_tail != 0;
    bz_prepare(io, T);
    const uint64_t n_waves = (uint64_t)gridDim.x * kGzWaves;
    for (uint64_t i = (uint64_t)blockIdx.x * kGzWaves + wv; i < J.n_chain; i += n_waves) {
        const uint64_t k = J.chain[i];
        io.sym = J.sym + J.off[i]; io.cap = J.off[i + 1] - J.off[i];
        // (a job's records lie at slots relative to its first element's; without slots — a seeded walk that meets records again — none is kept)
        if (MEM && J.slot) { io.ends = J.ends + (J.slot[i] - J.slot[0]); io.ends_cap = (uint32_t)(J.slot[i + 1] - J.slot[i]); }
        (void)gz_run<GZ_DECODE, MEM>(io, T, J.G, k, J.start[k], nullptr, J.end_bit[k]);
        io.sync();
    }
}
__global__ __launch_bounds__(64 * kGzWaves) void k_gz_decode(GzJob J)
{
    __shared__ BzTables tabs[kGzWaves];
    gz_decode_waves<false>(J, tabs);
}
__global__ __launch_bounds__(64 * kGzWaves) void k_gz_decode_members(GzJob J)
{
    __shared__ BzTables tabs[kGzWaves];
    gz_decode_waves<true>(J, tabs);
}

// element i's window needs element i - 1's: one workgroup, a barrier between elements
// A job that starts behind the file's element 0 (e0 > 0: the elements a rank of a group adds later, gzip_kept_grow) is SEEDED: win[0,
// 32768) holds the resolved window in front of its first element, and with n_win = n_chain the walk also leaves the window
// behind its last element in slot n_chain, the seed of the next walk.  Writes win[32768 i, 32768 (i + 1)) for i in [1, n_chain),
// or [1, n_win] where n_win is set
__global__ __launch_bounds__(kGzWindowThreads) void k_gz_windows(GzJob J)
{
    const uint64_t n = J.n_win ? J.n_win + 1 : J.n_chain;
    for (uint64_t i = 1; i < n; i++) {
        const uint16_t *sp = J.sym + J.off[i - 1];
        const uint64_t L = J.off[i] - J.off[i - 1];
        const uint8_t *wp = J.e0 + i > 1 ? J.win + (i - 1) * (uint64_t)kGzWindow : nullptr;
        uint8_t *w = J.win + i * (uint64_t)kGzWindow;
        for (uint32_t e = threadIdx.x; e < kGzWindow; e += kGzWindowThreads) w[e] = gz_window_entry(sp, L, wp, e);
        __syncthreads();                                  // (workgroup scope: the next element reads what all threads wrote)
    }
}

// the same walk over a range of the chain whose entry window is unknown: symbolic windows (gz_window_entry_sym) from the
// identity in front of the range's first element; ONE workgroup, a barrier between elements.  Writes wsym[32768 i, 32768 (i + 1))
// for i in [1, n_win] only
__global__ __launch_bounds__(kGzWindowThreads) void k_gz_windows_sym(GzJob J)
{
    for (uint64_t i = 1; i <= J.n_win; i++) {
        const uint16_t *sp = J.sym + J.off[i - 1];
        const uint64_t L = J.off[i] - J.off[i - 1];
        const uint16_t *wp = i > 1 ? J.wsym + (i - 1) * (uint64_t)kGzWindow : nullptr;
        uint16_t *w = J.wsym + i * (uint64_t)kGzWindow;
        for (uint32_t e = threadIdx.x; e < kGzWindow; e += kGzWindowThreads) w[e] = gz_window_entry_sym(sp, L, wp, e);
        __syncthreads();                                  // (workgroup scope: the next element reads what all threads wrote)
    }
}

// ... in members mode: entries that lie in front of the member that holds the element's first byte are dead and read 0
// (gunzip_core.h); m0[i] for i in [1, n_win] is read
__global__ __launch_bounds__(kGzWindowThreads) void k_gz_windows_sym_members(GzJob J)
{
    for (uint64_t i = 1; i <= J.n_win; i++) {
        const uint16_t *sp = J.sym + J.off[i - 1];
        const uint64_t L = J.off[i] - J.off[i - 1], t0 = J.off[i], m0 = J.m0[i];
        const uint16_t *wp = i > 1 ? J.wsym + (i - 1) * (uint64_t)kGzWindow : nullptr;
        uint16_t *w = J.wsym + i * (uint64_t)kGzWindow;
        for (uint32_t e = threadIdx.x; e < kGzWindow; e += kGzWindowThreads) w[e] = gz_window_entry_sym_members(sp, L, wp, e, t0, m0);
        __syncthreads();                                  // (workgroup scope: the next element reads what all threads wrote)
    }
}

// once the entry window has arrived in win[0, 32768): a workgroup per element, grid-stride, no order among them.  Writes
// win[32768 i, 32768 (i + 1)) for i in [1, n_win] only: win has n_win + 1 slots, the last one the window behind the range's last
// element where n_win = n_chain (a range that starts at the file's element 0 has no
// entry window: its markers point in front of the text and read 0, as in gz_window_entry)
__global__ __launch_bounds__(kGzWindowThreads) void k_gz_window_resolve(GzJob J)
{
    const uint8_t *entry = J.e0 ? J.win : nullptr;
    const uint64_t n = J.n_win + 1;
    for (uint64_t i = 1 + blockIdx.x; i < n; i += gridDim.x) {
        const uint16_t *ws = J.wsym + i * (uint64_t)kGzWindow;
        uint8_t *w = J.win + i * (uint64_t)kGzWindow;
        for (uint32_t e = threadIdx.x; e < kGzWindow; e += kGzWindowThreads) w[e] = gz_window_resolve(ws[e], entry);
    }
}

// (shared memory as parameters: one set per kernel)
template <bool MEM> __device__ __forceinline__ void gz_narrow_groups(const GzJob &J, uint32_t *crc_tab, uint32_t &crc_acc, uint32_t &bad_acc)
{
    if (!MEM) crc_tab[threadIdx.x & 255u] = bz_crc_entry(threadIdx.x & 255u);
    for (uint64_t i = blockIdx.x; i < J.n_chain; i += gridDim.x) {
        if (threadIdx.x == 0) { crc_acc = 0; bad_acc = 0; }
        __syncthreads();
        const uint64_t o0 = J.off[i], L = J.off[i + 1] - o0;
        const uint16_t *sp = J.sym + o0;
        const uint8_t *win = J.e0 + i ? J.win + i * (uint64_t)kGzWindow : nullptr;
        const uint64_t m0 = MEM ? J.m0[i] : 0;
        // vector by vector of the OUTPUT's aligned space: [lead, lead + L) of it is the element's
        const uint32_t lead = (uint32_t)(((uintptr_t)J.out + o0) & 15u);
        uint8_t *const a_out = J.out + o0 - lead;          // 16-byte aligned (only [lead, lead + L) of it is touched)
        const uint64_t end = lead + L, n_vec = (end + 15u) / 16u;
        uint32_t bad = 0;
        for (uint64_t v = threadIdx.x; v < n_vec; v += kGzNarrowThreads) {
            const uint64_t lo = v * 16u;
            if (lo >= lead && lo + 16u <= end) {
                uint32_t w[4] = {0, 0, 0, 0};
                for (uint32_t q = 0; q < 16u; q++) {
                    const uint32_t b = gz_narrow(sp[lo - lead + q], win, o0, m0);
                    bad |= b >> 8;
                    w[q >> 2] |= (b & 0xFFu) << (8u * (q & 3u));
                }
                *reinterpret_cast<uint4 *>(a_out + lo) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                for (uint64_t q = lo < lead ? lead : lo; q < lo + 16u && q < end; q++) {
                    const uint32_t b = gz_narrow(sp[q - lead], win, o0, m0);
                    bad |= b >> 8;
                    a_out[q] = (uint8_t)b;
                }
            }
        }
        if (bad) atomicOr(&bad_acc, 1u);
        __syncthreads();                                  // (workgroup scope: the slices below read what all threads stored)
        // the element's CRC-32: 256 slices, each one's CRC moved to its place by x^(8 bytes behind it), summed
        // (not in members mode: a member's CRC-32 is k_gz_member_crc's, elements do not end where members do; crc_tab and crc_acc
        // stay untouched there)
        if (!MEM) {
            const uint64_t per = (L + kGzNarrowThreads - 1) / kGzNarrowThreads;
            const uint64_t a = threadIdx.x * per < L ? threadIdx.x * per : L, b = a + per < L ? a + per : L;
            if (b > a) {
                const uint8_t *t = J.out + o0;
                uint32_t c = 0xFFFFFFFFu;
                for (uint64_t p = a; p < b; p++) c = crc_tab[(c ^ t[p]) & 0xFFu] ^ (c >> 8);
                atomicXor(&crc_acc, gz_crc_join(~c, 0u, L - b));
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (!MEM) J.crc_part[i] = crc_acc;
            if (bad_acc) atomicMin(J.verdict, (unsigned long long)i);
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(kGzNarrowThreads) void k_gz_narrow(GzJob J)
{
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t crc_acc, bad_acc;
    gz_narrow_groups<false>(J, crc_tab, crc_acc, bad_acc);
}
__global__ __launch_bounds__(kGzNarrowThreads) void k_gz_narrow_members(GzJob J)
{
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t crc_acc, bad_acc;
    gz_narrow_groups<true>(J, crc_tab, crc_acc, bad_acc);
}

// a wave per piece of text, grid-stride: every lane's slice of the piece, moved to its place by x^(8 bytes behind it), summed over
// the wave.  The table is the wave's own (no workgroup barrier); the text was stored by k_gz_narrow_members, a launch before
__global__ __launch_bounds__(64 * kGzWaves) void k_gz_member_crc(GzJob J)
{
    __shared__ uint32_t tabs[kGzWaves][256];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t *crc_tab = tabs[wv];
    for (uint32_t e = lane; e < 256u; e += 64u) crc_tab[e] = bz_crc_entry(e);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t n_waves = (uint64_t)gridDim.x * kGzWaves;
    for (uint64_t q = (uint64_t)blockIdx.x * kGzWaves + wv; q < J.n_pieces; q += n_waves) {
        const uint64_t p0 = J.piece[q], L = J.piece[q + 1] - p0;
        const uint64_t per = (L + 63u) / 64u;
        const uint64_t a = lane * per < L ? lane * per : L, b = a + per < L ? a + per : L;
        uint32_t part = 0;
        if (b > a) {
            const uint8_t *t = J.out + p0;
            uint32_t c = 0xFFFFFFFFu;
            for (uint64_t p = a; p < b; p++) c = crc_tab[(c ^ t[p]) & 0xFFu] ^ (c >> 8);
            part = gz_crc_join(~c, 0u, L - b);
        }
        for (int m = 32; m; m >>= 1) part ^= __shfl_xor(part, m, 64);
        if (lane == 0) J.crc_piece[q] = part;
    }
}

static hipError_t gz_grid(uint64_t n_items, int per_group, int groups_per_cu, unsigned *grid)
{
    int dev = 0, n_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const uint64_t want = (n_items + per_group - 1) / per_group;
    *grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)groups_per_cu * (uint64_t)std::max(n_cu, 1)));
    return hipSuccess;
}

hipError_t launch_gz_find(const GzJob &J, hipStream_t st, bool members)
{
    unsigned grid = 1;
    hipError_t e = gz_grid(J.k1 - J.k0, kGzWaves, 4, &grid);
    if (e != hipSuccess) return e;
    if (members) CRASS_LAUNCH(k_gz_find_members, dim3(grid), dim3(64 * kGzWaves), 0, st, J);
    else CRASS_LAUNCH(k_gz_find, dim3(grid), dim3(64 * kGzWaves), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_gz_count(const GzJob &J, hipStream_t st, bool members)
{
    unsigned grid = 1;
    hipError_t e = gz_grid(J.k1 - J.k0, kGzWaves, 4, &grid);
    if (e != hipSuccess) return e;
    if (members) CRASS_LAUNCH(k_gz_count_members, dim3(grid), dim3(64 * kGzWaves), 0, st, J);
    else CRASS_LAUNCH(k_gz_count, dim3(grid), dim3(64 * kGzWaves), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_gz_decode(const GzJob &J, hipStream_t st, bool members)
{
    if (J.n_chain == 0) return hipSuccess;
    unsigned grid = 1;
    hipError_t e = gz_grid(J.n_chain, kGzWaves, 4, &grid);
    if (e != hipSuccess) return e;
    if (members) CRASS_LAUNCH(k_gz_decode_members, dim3(grid), dim3(64 * kGzWaves), 0, st, J);
    else CRASS_LAUNCH(k_gz_decode, dim3(grid), dim3(64 * kGzWaves), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_gz_windows(const GzJob &J, hipStream_t st)
{
    if ((J.n_win ? J.n_win + 1 : J.n_chain) < 2) return hipSuccess;
    CRASS_LAUNCH(k_gz_windows, dim3(1), dim3(kGzWindowThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_gz_windows_sym(const GzJob &J, hipStream_t st, bool members)
{
    if (J.n_win == 0) return hipSuccess;
    if (members) CRASS_LAUNCH(k_gz_windows_sym_members, dim3(1), dim3(kGzWindowThreads), 0, st, J);
    else CRASS_LAUNCH(k_gz_windows_sym, dim3(1), dim3(kGzWindowThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_gz_window_resolve(const GzJob &J, hipStream_t st)
{
    const uint64_t n = J.n_win + 1;
    if (n < 2) return hipSuccess;
    unsigned grid = 1;
    hipError_t e = gz_grid(n - 1, 1, 2, &grid);
    if (e != hipSuccess) return e;
    CRASS_LAUNCH(k_gz_window_resolve, dim3(grid), dim3(kGzWindowThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_gz_narrow(const GzJob &J, hipStream_t st, bool members)
{
    if (J.n_chain == 0) return hipSuccess;
    unsigned grid = 1;
    hipError_t e = gz_grid(J.n_chain, 1, 8, &grid);
    if (e != hipSuccess) return e;
    if (members) CRASS_LAUNCH(k_gz_narrow_members, dim3(grid), dim3(kGzNarrowThreads), 0, st, J);
    else CRASS_LAUNCH(k_gz_narrow, dim3(grid), dim3(kGzNarrowThreads), 0, st, J);
    return hipGetLastError();
}

hipError_t launch_gz_member_crc(const GzJob &J, hipStream_t st)
{
    if (J.n_pieces == 0) return hipSuccess;
    unsigned grid = 1;
    hipError_t e = gz_grid(J.n_pieces, kGzWaves, 4, &grid);
    if (e != hipSuccess) return e;
    CRASS_LAUNCH(k_gz_member_crc, dim3(grid), dim3(64 * kGzWaves), 0, st, J);
    return hipGetLastError();
}

} // namespace crass
