// Issue-rate microbenchmark for the VALU instructions the scan kernels are built from.
// 6 blocks x 4 waves per CU, 8 independent dependency chains per lane, inline asm so the
// compiler cannot substitute instructions.  Prints cycles per wave-instruction per SIMD.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define CHAINS 8
#define BODY(ASM) \
  for (int it = 0; it < iters; it++) { \
    _Pragma("unroll") for (int i = 0; i < CHAINS; i++) { asm volatile(ASM : "+v"(a[i]) : "v"(b[i]), "v"(c) ); } }
template<int OP> __global__ void k(uint32_t* out, int iters){
  uint32_t a[CHAINS], b[CHAINS]; uint32_t c = threadIdx.x * 2654435761u + 12345u;
  for (int i=0;i<CHAINS;i++){ a[i]=c+i*77u; b[i]=c*3+i; }
  if (OP==0)  BODY("v_xor_b32 %0, %0, %1")
  if (OP==1)  BODY("v_pk_min_u16 %0, %0, %1")
  if (OP==2)  BODY("v_pk_sub_u16 %0, %0, %1")
  if (OP==3)  BODY("v_pk_add_u16 %0, %0, %1")
  if (OP==4)  BODY("v_min_u32 %0, %0, %1")
  if (OP==5)  BODY("v_add_u32 %0, %0, %1")
  if (OP==6)  BODY("v_and_or_b32 %0, %0, %1, %2")
  if (OP==7)  BODY("v_bfi_b32 %0, %0, %1, %2")
  if (OP==8)  BODY("v_alignbit_b32 %0, %0, %1, 6")
  if (OP==9)  BODY("v_alignbyte_b32 %0, %0, %1, 1")
  if (OP==10) BODY("v_perm_b32 %0, %0, %1, %2")
  if (OP==11) BODY("v_lshl_or_b32 %0, %0, 3, %1")
  if (OP==12) BODY("v_or3_b32 %0, %0, %1, %2")
  if (OP==13) BODY("v_mul_u32_u24 %0, %0, %1")
  if (OP==14) BODY("v_mad_u32_u24 %0, %0, %1, %2")
  if (OP==15) BODY("v_sad_u16 %0, %0, %1, %2")
  if (OP==16) BODY("v_msad_u8 %0, %0, %1, %2")
  if (OP==17) BODY("v_cmp_eq_u32 vcc, %0, %1\n v_addc_co_u32 %0, vcc, 0, %0, vcc")
  if (OP==18) BODY("v_cmp_eq_u16_sdwa vcc, %0, %1 src0_sel:WORD_0 src1_sel:WORD_1\n v_addc_co_u32 %0, vcc, 0, %0, vcc")
  if (OP==19) BODY("v_lshrrev_b32 %0, 3, %0")
  if (OP==20) BODY("v_sub_u32 %0, %0, %1")
  if (OP==21) BODY("v_max_u32 %0, %0, %1")
  if (OP==22) BODY("v_and_b32 %0, %0, %1")
  if (OP==23) BODY("v_bfe_u32 %0, %0, 3, 5")
  if (OP==24) BODY("v_lshl_add_u32 %0, %0, 2, %1")
  if (OP==25) BODY("v_min_u16 %0, %0, %1")
  if (OP==26) BODY("v_pk_max_u16 %0, %0, %1")
  if (OP==27) BODY("v_cndmask_b32 %0, %0, %1, vcc")
  // gfx950 only.  bitop3:0x28 = (src0 ^ src1) & src2.  The f16 rows feed minimum3 masked halfwords only (sign 0, exponent below
  // all-ones: no NaN / Inf operand), as the seed scan would.
  if (OP==28) BODY("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x28")
  if (OP==29) { c = 0x3FFF3FFFu; for (int i=0;i<CHAINS;i++){ a[i]&=c; b[i]&=c; } BODY("v_pk_minimum3_f16 %0, %0, %1, %2") }
  // the scan's dependent groups, per two (word, shift) pairs: 3 instructions (new) against 4 (today's)
  if (OP==30) { const uint32_t m = 0x3FFF3FFFu; for (int i=0;i<CHAINS;i++) a[i]&=m;
    for (int it = 0; it < iters; it++) { _Pragma("unroll") for (int i = 0; i < CHAINS; i++) { uint32_t t0, t1;
      asm volatile("v_bitop3_b32 %1, %3, %4, %5 bitop3:0x28\n v_bitop3_b32 %2, %4, %3, %5 bitop3:0x28\n v_pk_minimum3_f16 %0, %0, %1, %2"
                   : "+v"(a[i]), "=&v"(t0), "=&v"(t1) : "v"(b[i]), "v"(c), "v"(m)); } } }
  if (OP==31) {
    for (int it = 0; it < iters; it++) { _Pragma("unroll") for (int i = 0; i < CHAINS; i++) { uint32_t t0, t1;
      asm volatile("v_xor_b32 %1, %3, %4\n v_pk_min_u16 %0, %0, %1\n v_xor_b32 %2, %4, %3\n v_pk_min_u16 %0, %0, %2"
                   : "+v"(a[i]), "=&v"(t0), "=&v"(t1) : "v"(b[i]), "v"(c)); } } }
  uint32_t s=0; for(int i=0;i<CHAINS;i++) s^=a[i]; out[blockIdx.x*blockDim.x+threadIdx.x]=s;
}
template<int OP> float run(uint32_t* d, int iters){ hipEvent_t e0,e1; hipEventCreate(&e0); hipEventCreate(&e1); float best=1e9;
  for(int rep=0;rep<3;rep++){ hipEventRecord(e0); hipLaunchKernelGGL(k<OP>, dim3(256*6), dim3(256), 0, 0, d, iters); hipEventRecord(e1); hipEventSynchronize(e1); float ms; hipEventElapsedTime(&ms,e0,e1); if(ms<best) best=ms; } return best; }
// What v_pk_minimum3_f16 makes of the halfwords the seed scan would give it, in the mode a kernel of this build starts in
// (mode = 0) and with FP_DENORM set to "keep" for every format by the kernel itself (mode = 1).  Every pair (i, j) of masked
// halfwords 0 .. 0x3FFF (zero, every f16 denormal 0x0001 .. 0x03FF, every normal up to exponent 0b01111) and a third operand
// derived from them: the result must be the UNSIGNED minimum in both halves, or the loose filter is no superset.
static __device__ __forceinline__ uint32_t pk_minimum3(uint32_t a, uint32_t b, uint32_t c)
{
  uint32_t r; asm volatile("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
}
__global__ void k_min3_check(unsigned long long* bad, uint32_t* probe, int mode){
  if (mode) asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 4, 4), 0xf");
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;     // 0 .. 0x3FFF
  unsigned long long n = 0;
  for (uint32_t j = 0; j < 0x4000u; j++) {
    const uint32_t t = (i * 40503u + j * 9973u) & 0x3FFFu;
    const uint32_t r = pk_minimum3(i | (j << 16), j | (t << 16), t | (i << 16));
    const uint32_t m = i < j ? (i < t ? i : t) : (j < t ? j : t);
    n += (r & 0xFFFFu) != m; n += (r >> 16) != m;
  }
  if (n) atomicAdd(bad, n);
  if (i == 0) {   // the cases by name: denormals against zero and against each other, accumulator start 0x3C00
    probe[0] = pk_minimum3(0x3C003C00u, 0x00010001u, 0x03FF03FFu);   // want 0x00010001
    probe[1] = pk_minimum3(0x3C003C00u, 0x00010000u, 0x03FF03FFu);   // want 0x00010000
    probe[2] = pk_minimum3(0x00010001u, 0x3C003FFFu, 0x3FFF3C00u);   // want 0x00010001
    probe[3] = pk_minimum3(0x3C003C00u, 0x3FFF3BFFu, 0x3FFF3FFFu);   // want 0x3C003BFF
  }
}
static void min3_check(){ unsigned long long* bad; uint32_t* probe; hipMalloc(&bad, 8); hipMalloc(&probe, 16);
  for (int mode = 0; mode < 2; mode++) { unsigned long long hb = 0; uint32_t hp[4];
    hipMemset(bad, 0, 8); hipMemset(probe, 0xEE, 16);
    hipLaunchKernelGGL(k_min3_check, dim3(64), dim3(256), 0, 0, bad, probe, mode); hipDeviceSynchronize();
    hipMemcpy(&hb, bad, 8, hipMemcpyDeviceToHost); hipMemcpy(hp, probe, 16, hipMemcpyDeviceToHost);
    printf("v_pk_minimum3_f16 vs unsigned min, 2^28 masked halfword triples x 2 halves, %s: %llu mismatches; probes %08x %08x %08x %08x (want 00010001 00010000 00010001 3c003bff)\n",
           mode ? "FP_DENORM=0xf set by the kernel" : "kernel start mode", hb, hp[0], hp[1], hp[2], hp[3]); }
  hipFree(bad); hipFree(probe); }
int main(){ uint32_t* d; hipMalloc(&d, 256*6*256*4); const int iters=4000;
 const char* names[]={"v_xor_b32","v_pk_min_u16","v_pk_sub_u16","v_pk_add_u16","v_min_u32","v_add_u32","v_and_or_b32","v_bfi_b32","v_alignbit_b32","v_alignbyte_b32","v_perm_b32","v_lshl_or_b32","v_or3_b32","v_mul_u32_u24","v_mad_u32_u24","v_sad_u16","v_msad_u8","v_cmp_eq_u32+v_addc","v_cmp_eq_u16_sdwa+v_addc","v_lshrrev_b32","v_sub_u32","v_max_u32","v_and_b32","v_bfe_u32","v_lshl_add_u32","v_min_u16","v_pk_max_u16","v_cndmask_b32","v_bitop3_b32","v_pk_minimum3_f16","2 v_bitop3 + v_pk_minimum3_f16","2 (v_xor + v_pk_min_u16)"};
 const int ninstr[]={1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,2,2,1,1,1,1,1,1,1,1,1,1,1,3,4};
 float ms[32];
 ms[0]=run<0>(d,iters); ms[1]=run<1>(d,iters); ms[2]=run<2>(d,iters); ms[3]=run<3>(d,iters); ms[4]=run<4>(d,iters); ms[5]=run<5>(d,iters); ms[6]=run<6>(d,iters); ms[7]=run<7>(d,iters);
 ms[8]=run<8>(d,iters); ms[9]=run<9>(d,iters); ms[10]=run<10>(d,iters); ms[11]=run<11>(d,iters); ms[12]=run<12>(d,iters); ms[13]=run<13>(d,iters); ms[14]=run<14>(d,iters); ms[15]=run<15>(d,iters);
 ms[16]=run<16>(d,iters); ms[17]=run<17>(d,iters); ms[18]=run<18>(d,iters); ms[19]=run<19>(d,iters); ms[20]=run<20>(d,iters); ms[21]=run<21>(d,iters); ms[22]=run<22>(d,iters); ms[23]=run<23>(d,iters);
 ms[24]=run<24>(d,iters); ms[25]=run<25>(d,iters); ms[26]=run<26>(d,iters); ms[27]=run<27>(d,iters);
 ms[28]=run<28>(d,iters); ms[29]=run<29>(d,iters); ms[30]=run<30>(d,iters); ms[31]=run<31>(d,iters);
 for(int op=0;op<32;op++){ double n = 256.0*6*4*iters*CHAINS*ninstr[op]; double per_simd = n/(256*4); printf("%-28s %.3f ms  %.2f cycles/instr/SIMD (@2.4GHz nominal)\n", names[op], ms[op], ms[op]*1e-3*2.4e9/per_simd); }
 min3_check();
 return 0; }
