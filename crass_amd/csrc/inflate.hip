// inflate.hip — BGZF members inflated on the device: k_bgzf_inflate, one wave per member, kBzWaves waves per workgroup, a
// grid-stride walk over the members.  The decoder is inflate_core.h's, statement for statement what the host runs (bgzf.cpp);
// this file only says how a wave goes through it:
//   * symbol decoding is serial: all 64 lanes run it with the same values (no lane waits for another, no broadcast)
//   * the code tables, the match copies (overlapping ones too: byte i comes from pos - dist + i mod dist), stored runs and the
//     CRC-32 (64 slices, each moved to its place by x^(8 bytes behind it) mod P) are io.par: lane l takes i = l, l + 64, ...
//   * where the member's text lives while it is decoded is a template parameter, both placements are built and timed
//     (profiles/NOTES_r14.md: 20 GB/s of text in HBM against 3.2 in LDS, so the HBM placement is the default and
//     CRASS_INFLATE_WINDOW=lds, read when the context is created, selects the other):
//       LDS   the wave's 64 KB window of LDS, at the offset the member's first byte has in its 16-byte vector of the output; the
//             text leaves in aligned 16-byte stores, byte stores only in the member's first and last partial vector.  Two windows
//             and two sets of tables (6.5 KB) per workgroup: 141 KB of the CU's 160 KB, two members per CU.
//       HBM   the member's own range of the output: literals and
//             match bytes are stored there as they are decoded and back-references are loaded from there.  Only the tables are
//             in LDS: four waves per workgroup, the registers decide how many members a CU holds.
//   * what a lane wrote — to LDS, or in the HBM placement to the member's range of the output — is read by other lanes of the SAME
//     wave only.  The LLVM AMDGPU memory model (AMDGPUUsage, "Memory Model", gfx90a / gfx942: the LDS and vector memory operations
//     of one wavefront are issued and complete in program order, so a fence at WAVEFRONT scope needs no wait and no cache
//     action) makes a release / acquire fence at that scope all that ordering between lanes of a wave takes; so io.sync()
//     is a wavefront-scope fence plus a wave barrier — both for the compiler,
//     neither is an instruction.  No other wave ever reads a member's range during the launch.
// Input is read inside [in + data_off[m], in + in_off[m + 1]) only (in() checks the index), output is written inside
// [out + out_off[m], out + out_off[m + 1]) only (LDS placement: only for a member that was accepted; HBM placement: a declined
// member leaves what it had decoded, inside its range); a text index is checked against the member's ISIZE in put() and get().
// A declined member writes its reason, min-s its offence into the verdict and stops;
// the others go on.  No workgroup barrier: the waves of a workgroup never wait for each other.
#include "inflate_launch.h"
#include "engine_internal.h"
#include "devmem.h"

namespace crass {

static constexpr int kBzWaves = 2, kBzWavesHbm = 4;                        // waves per workgroup: LDS placement, HBM placement
static constexpr uint32_t kBzWinBytes = kBzMaxText + 16;                   // a member's text behind a lead of 0 .. 15 bytes
static constexpr uint32_t kBzTabBytes = (sizeof(BzTables) + 15u) & ~15u;
static constexpr uint32_t kBzLdsBytes = kBzWaves * (kBzWinBytes + kBzTabBytes), kBzLdsBytesHbm = kBzWavesHbm * kBzTabBytes;
static_assert(kBzWinBytes % 16 == 0 && kBzLdsBytes <= 160 * 1024, "two windows and two sets of tables fit a CU's LDS");

struct BzWaveIO {
    const uint8_t *src; uint32_t n_in; uint8_t *win; uint32_t isize; uint32_t lane;
    __device__ __forceinline__ uint32_t in(uint32_t i) const { return i < n_in ? (uint32_t)src[i] : 0u; }
    __device__ __forceinline__ void put(uint32_t p, uint32_t b) { if (p < isize) win[p] = (uint8_t)b; }
    __device__ __forceinline__ uint32_t get(uint32_t p) const { return p < isize ? (uint32_t)win[p] : 0u; }
    template <class F> __device__ __forceinline__ void par(uint32_t n, F f) { for (uint32_t i = lane; i < n; i += 64u) f(i); }
    __device__ __forceinline__ bool lead() const { return lane == 0; }
    __device__ __forceinline__ void sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

// WAVES waves per workgroup; LDS_WINDOW: the text in the wave's LDS window (else in the member's range of the output)
template <int WAVES, bool LDS_WINDOW> __global__ __launch_bounds__(64 * WAVES) void k_bgzf_inflate(BzJob J)
{
    extern __shared__ uint4 bz_lds[];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint8_t *const lds = reinterpret_cast<uint8_t *>(bz_lds);
    uint8_t *const window = lds + wv * kBzWinBytes;       // (LDS placement only)
    BzTables &T = *reinterpret_cast<BzTables *>(lds + (LDS_WINDOW ? WAVES * kBzWinBytes : 0u) + wv * kBzTabBytes);
    {
        BzWaveIO io{nullptr, 0, nullptr, 0, lane};
        bz_prepare(io, T);
    }
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t m = (uint64_t)blockIdx.x * WAVES + wv; m < J.n_members; m += n_waves) {
        const uint64_t d0 = J.data_off[m], e0 = J.in_off[m + 1] - 8, o0 = J.out_off[m];      // (the engine checked: d0 <= e0, e0 - d0 <= 65536)
        const uint32_t isize = (uint32_t)(J.out_off[m + 1] - o0);                          // (... and isize <= 65536)
        const uint32_t lead = (uint32_t)(((uintptr_t)J.out + o0) & 15u);
        BzWaveIO io{J.in + d0, (uint32_t)(e0 - d0), LDS_WINDOW ? window + lead : J.out + o0, isize, lane};
        int32_t why = bz_inflate_member(io, T, io.n_in, isize);
        if (why == BZ_OK) {
            const uint8_t *t = J.in + e0;                  // the trailer: CRC-32, ISIZE
            const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            if (bz_text_crc(io, T, isize) != crc) why = BZ_CRC;
        }
        if (lane == 0) {
            J.reason[m] = (uint32_t)why;
            if (why != BZ_OK) atomicMin(J.verdict, (unsigned long long)bz_offence(m, (uint32_t)why));
        }
        if (LDS_WINDOW && why == BZ_OK) {
            // the window, vector by vector of the OUTPUT's aligned space: [lead, lead + isize) of it is the member's
            uint8_t *const a_out = J.out + o0 - lead;      // 16-byte aligned
            const uint32_t end = lead + isize, n_vec = (end + 15u) / 16u;
            for (uint32_t v = lane; v < n_vec; v += 64u) {
                const uint32_t lo = v * 16u;
                if (lo >= lead && lo + 16u <= end) {
                    *reinterpret_cast<uint4 *>(a_out + lo) = *reinterpret_cast<const uint4 *>(window + lo);
                } else {
                    for (uint32_t q = lo < lead ? lead : lo; q < lo + 16u && q < end; q++) a_out[q] = window[q];
                }
            }
        }
        io.sync();                                         // (the window's next member starts when this one has left)
    }
}

hipError_t launch_bgzf_inflate(const BzJob &J, hipStream_t st)
{
    if (J.n_members == 0) return hipSuccess;
    int dev = 0, n_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (J.hbm_window) {
        // five workgroups per CU: 20 waves, what the kernel's 94 VGPRs admit
        const uint64_t want = (J.n_members + kBzWavesHbm - 1) / kBzWavesHbm;
        const unsigned grid = (unsigned)std::min<uint64_t>(want, 5ull * (uint64_t)std::max(n_cu, 1));
        CRASS_LAUNCH((k_bgzf_inflate<kBzWavesHbm, false>), dim3(grid), dim3(64 * kBzWavesHbm), kBzLdsBytesHbm, st, J);
        return hipGetLastError();
    }
    // one workgroup per CU fills the LDS; fewer members than that: a workgroup per kBzWaves members
    const uint64_t want = (J.n_members + kBzWaves - 1) / kBzWaves;
    const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)std::max(n_cu, 1));
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bgzf_inflate<kBzWaves, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBzLdsBytes);
    if (e != hipSuccess) return e;
    CRASS_LAUNCH((k_bgzf_inflate<kBzWaves, true>), dim3(grid), dim3(64 * kBzWaves), kBzLdsBytes, st, J);
    return hipGetLastError();
}

} // namespace crass
