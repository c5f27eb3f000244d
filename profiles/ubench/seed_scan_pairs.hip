// The pass-1 seed scan's inner loop at 150 bp (W = 10, shifts 49 .. 97, length clamp), as k_filter_fast_impl runs it (EXACT:
// v_alignbit + v_xor + v_pk_min_u16 per word and shift) and with two shifts folded per minimum (LOOSE: v_alignbit + two
// v_bitop3_b32 (s ^ w) & 0x3FFF3FFF + one v_pk_minimum3_f16), on rows made up in registers: no memory traffic, no recheck of the
// loose positives, no hint.  What the pairing can save of the scan's VALU time at most.  6 blocks x 4 waves per CU as
// valu_rate_asm.hip; prints ms and cycles per row and wave at the nominal 2.4 GHz.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
  u16x2 r = __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
  return __builtin_bit_cast(uint32_t, r);
}
static __device__ __forceinline__ uint32_t bitop3_xor_and(uint32_t a, uint32_t b, uint32_t m)
{
  uint32_t r; asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x28" : "=v"(r) : "v"(a), "v"(b), "v"(m)); return r;
}
static __device__ __forceinline__ uint32_t pk_minimum3_f16(uint32_t a, uint32_t b, uint32_t c)
{
  uint32_t r; asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
}
constexpr int W = 10, D0 = 49, D1 = 97, LCT = 150, WX = W + (D1 >> 4) + 2, SW = ((16 * W - 58) / 8 + 2) / 2;
static __device__ __forceinline__ uint32_t shifted(const uint32_t (&w)[WX], int k, int d)
{
  const int q = d >> 4, sh = (d & 15) * 2;
  return sh ? __builtin_amdgcn_alignbit(w[k + q + 1], w[k + q], sh) : w[k + q];
}
template <int LOOSE> __global__ __launch_bounds__(256) void k_scan(uint32_t *out, int rows)
{
  uint32_t w[WX], base[W], sum = 0;
  uint32_t seed = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u;
  for (int i = 0; i < W; i++) { seed = seed * 1664525u + 1013904223u; base[i] = seed; }
  const uint32_t m = 0x3FFF3FFFu;
  for (int it = 0; it < rows; it++) {
#pragma unroll
    for (int i = 0; i < WX; i++) w[i] = i < W ? base[i] + (uint32_t)it * 0x9E3779B9u : 0u;     // (a new row: one add per word)
    uint32_t acc[SW];
#pragma unroll
    for (int i = 0; i < SW; i++) acc[i] = LOOSE ? 0x3C003C00u : 0xFFFFFFFFu;
    if (LOOSE) {
#pragma unroll
      for (int d = D0; d <= D1; d += 2) {
#pragma unroll
        for (int k = 0; k < SW; k++) {
          if (d > LCT - 9 - 16 * k) continue;
          const uint32_t a = bitop3_xor_and(shifted(w, k, d), w[k], m);
          const bool two = d + 1 <= D1 && d + 1 <= LCT - 9 - 16 * k;
          const uint32_t b = two ? bitop3_xor_and(shifted(w, k, d + 1), w[k], m) : a;
          acc[k] = pk_minimum3_f16(acc[k], a, b);
        }
      }
    } else {
#pragma unroll
      for (int d = D0; d <= D1; d++) {
#pragma unroll
        for (int k = 0; k < SW; k++) {
          if (d > LCT - 9 - 16 * k) continue;
          acc[k] = pk_min_u16(acc[k], shifted(w, k, d) ^ w[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < SW; k++) sum += acc[k];
  }
  out[blockIdx.x * 256u + threadIdx.x] = sum;
}
template <int LOOSE> static float run(uint32_t *d, int rows)
{
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); float best = 1e9f;
  for (int rep = 0; rep < 4; rep++) {
    (void)hipEventRecord(e0); hipLaunchKernelGGL(k_scan<LOOSE>, dim3(256 * 6), dim3(256), 0, 0, d, rows); (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1); float ms; (void)hipEventElapsedTime(&ms, e0, e1); if (rep && ms < best) best = ms;
  }
  return best;
}
int main()
{
  uint32_t *d; if (hipMalloc(&d, 256 * 6 * 256 * 4) != hipSuccess) return 1;
  const int rows = 256;
  for (int round = 0; round < 3; round++) {
    const float e = run<0>(d, rows), l = run<1>(d, rows);
    const double per_simd = 6.0 * rows;      // rows per SIMD: 6 blocks x 4 waves per CU, one wave of each block per SIMD
    printf("round %d: exact %.3f ms (%.0f cycles/row/wave)  loose %.3f ms (%.0f cycles/row/wave)  loose/exact %.3f\n", round,
           e, e * 1e-3 * 2.4e9 / per_simd, l, l * 1e-3 * 2.4e9 / per_simd, l / e);
  }
  return hipFree(d) != hipSuccess;
}
