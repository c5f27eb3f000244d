// dev_common.h — device functions shared by the kernel files (pass 1's, sinks.hip, pass2.hip): the wave helpers and the
// accessors of a resident read set.  Everything here is static and force-inlined; a function used by one file only lives there,
// and what only pass 1's files share is in search_bits.h.
#pragma once
#include "engine_internal.h"

namespace crass {

#define WAVE 64

static __device__ __forceinline__ void wave_sync()
{
    // LDS traffic of one wave is executed in order; this only stops the compiler from
    // moving LDS accesses across the point where lanes exchange data through LDS.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A value that is the same in every lane but was read from LDS (or computed from such a read) lives in a VGPR as far as the
// compiler knows, and everything derived from it — loop counters, branch conditions — becomes vector arithmetic under exec
// masks.  The wave-per-read kernel's control flow is wave-uniform throughout: naming the value once puts it, and what follows
// from it, on the scalar unit.
static __device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
static __device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
static __device__ __forceinline__ uint64_t uni64(uint64_t x) { return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | (uint64_t)uni((uint32_t)x); }

static __device__ __forceinline__ uint64_t rd_word_off(const DevReads &R, uint64_t r)
{
    return R.stride_words ? r * (uint64_t)R.stride_words : R.word_off[r];
}
static __device__ __forceinline__ uint32_t rd_len(const DevReads &R, uint64_t r)
{
    return R.uniform_len ? R.uniform_len : R.lengths[r];
}
static __device__ __forceinline__ bool rd_is_exc(const DevReads &R, uint64_t r)
{
    return (R.exc_mask[r >> 5] >> (r & 31)) & 1u;
}
// first word of read r's position hints: reads of one length need no table look-up (a dependent global load per read in the
// wave kernel's prefetch otherwise)
static __device__ __forceinline__ uint64_t rd_hint_off(const DevReads &R, uint64_t r)
{
    return R.uniform_len ? r * (uint64_t)((R.uniform_len + 63u) >> 6) : R.pos_hint_off[r];
}
static __device__ __forceinline__ uint64_t rd_header_id(const DevReads &R, uint64_t r)
{
    return R.header_id ? R.header_id[r] : r;
}

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
    u16x2 r = __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));   // v_pk_min_u16
    return __builtin_bit_cast(uint32_t, r);
}

} // namespace crass
