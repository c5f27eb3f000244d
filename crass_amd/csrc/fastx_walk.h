// fastx_walk.h — how the kernels of fastx_hid.hip and fastx_lines.hip read a header line's bytes, and how they are launched.
// Device code: only .hip files include this.
//
// A NAME is the bytes behind the record's header character up to the first isspace() byte (' ', '\t' .. '\r') or the input's end.
// Names lie at any byte offset: they are read as ALIGNED dwords, funnel-shifted into name-relative dwords (v_alignbyte_b32), so a
// name's hash and the comparison of two names do not depend on where they lie.  No byte below bytes or at / beyond bytes + n_bytes
// is read: the one dword that holds the input's first byte and the one that holds its last are loaded byte by byte (nm_ld4).
#pragma once
#include "fastx_names_launch.h"
#include "devmem.h"

namespace crass {

static constexpr int kNmThreads = 256;

// the aligned dword at address q of the input [lo, hi); bytes outside the input read as 0 and are not touched
static __device__ __forceinline__ uint32_t nm_ld4(uintptr_t lo, uintptr_t hi, uintptr_t q)
{
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const uint32_t *>(q);
    uint32_t w = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) { const uintptr_t a = q + j; if (a >= lo && a < hi) w |= (uint32_t)*reinterpret_cast<const uint8_t *>(a) << (8 * j); }
    return w;
}

// the input's bytes from a position on, four at a time (byte 0 lowest); one aligned load per step
struct NmCur {
    uintptr_t lo, hi, q;
    uint32_t w0, sh;
    uint64_t left;                   // bytes from here to the input's end
    __device__ __forceinline__ void init(uintptr_t lo_, uintptr_t hi_, uint64_t pos)      // pos <= hi - lo
    {
        lo = lo_; hi = hi_;
        const uintptr_t a = lo + pos;
        sh = (uint32_t)(a & 3u); q = a - sh; left = hi - a;
        w0 = left ? nm_ld4(lo, hi, q) : 0u;
    }
    __device__ __forceinline__ uint32_t next(uint32_t *avail)      // *avail: how many of the four bytes are inside the input
    {
        const uint32_t w1 = left > 4u - sh ? nm_ld4(lo, hi, q + 4) : 0u;
        const uint32_t w = __builtin_amdgcn_alignbyte(w1, w0, sh);
        *avail = left < 4 ? (uint32_t)left : 4u;
        w0 = w1; q += 4; left -= *avail;
        return w;
    }
};
// the four bytes at a position, without a cursor (the wave kernels: a dword per lane)
static __device__ __forceinline__ uint32_t nm_dword_at(uintptr_t lo, uintptr_t hi, uint64_t pos, uint32_t *avail)
{
    if (pos >= hi - lo) { *avail = 0; return 0u; }
    NmCur c;
    c.init(lo, hi, pos);
    return c.next(avail);
}

static __device__ __forceinline__ uint32_t nm_is_space(uint32_t c) { return (uint32_t)(c - 9u < 5u) | (uint32_t)(c == 32u); }
// how many of the first `avail` bytes of w come before the first isspace() byte / the first '\n'
static __device__ __forceinline__ uint32_t nm_name_bytes(uint32_t w, uint32_t avail)
{
    uint32_t stop = 1u << avail;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) stop |= nm_is_space((w >> (8 * j)) & 0xFFu) << j;
    return (uint32_t)__builtin_ctz(stop);
}
static __device__ __forceinline__ uint32_t nm_line_bytes(uint32_t w, uint32_t avail)
{
    uint32_t stop = 1u << avail;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) stop |= (uint32_t)(((w >> (8 * j)) & 0xFFu) == 10u) << j;
    return (uint32_t)__builtin_ctz(stop);
}
static __device__ __forceinline__ uint32_t nm_low_bytes(uint32_t cnt) { return cnt >= 4 ? 0xFFFFFFFFu : (1u << (8 * cnt)) - 1u; }

// one lane walks from pos of the input [lo, lo + n_bytes) (pos <= n_bytes): the name's bytes and, with LINE, the bytes up to the
// '\n' or the input's end — both from the one pass ('\n' is a space: the name ends no later than the line).  Without LINE the walk
// ends with the name and line stays 0.
struct NmSpan { uint64_t name, line; };
template <bool LINE> static __device__ __forceinline__ NmSpan nm_walk(uintptr_t lo, uint64_t n_bytes, uint64_t pos)
{
    NmCur c;
    c.init(lo, lo + n_bytes, pos);
    NmSpan s{0, 0};
    bool named = false;
    for (;;) {
        uint32_t avail;
        const uint32_t w = c.next(&avail);
        if (!named) { const uint32_t nb = nm_name_bytes(w, avail); s.name += nb; named = nb < 4; }
        if (LINE) {
            const uint32_t lb = nm_line_bytes(w, avail);
            s.line += lb;
            if (lb < 4) break;
        } else if (named) break;
    }
    return s;
}
// a length as the 32-bit arrays hold it
static __device__ __forceinline__ uint32_t nm_len32(uint64_t len) { return len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len; }

// ---- host: a launch of kNmThreads per block over `items`, per_block of them a block; no block, or more than 2^31 - 1: an error ----
static bool nm_grid(uint64_t items, uint64_t per_block, unsigned *blocks)
{
    const uint64_t g = (items + per_block - 1) / per_block;
    if (!g || g > 0x7FFFFFFFull) return false;
    *blocks = (unsigned)g;
    return true;
}
template <class K, class... A> static hipError_t nm_launch(const char *name, K kernel, uint64_t items, uint64_t per_block, hipStream_t st, const A &...args)
{
    unsigned g;
    if (!nm_grid(items, per_block, &g)) return hipErrorInvalidValue;
    CRASS_LAUNCH_AS(name, kernel, dim3(g), dim3(kNmThreads), 0, st, args...);
    return hipGetLastError();
}
#define NM_LAUNCH(kernel, ...) nm_launch(#kernel, kernel, __VA_ARGS__)      // (the name: CRASS_TRACE_LAUNCHES prints it)

} // namespace crass
