// Issue rate of the 64-bit shift forms (gfx950) against the 32-bit VOP2
// shift: can one v_lshrrev_b64 produce the shifted values of two 32-bit
// registers at the cost of one instruction?  8 independent chains per lane,
// 1024-thread workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

template <int OP>
__global__ __launch_bounds__(1024) void k(uint32_t* out, uint32_t iters, uint32_t seed) {
  uint64_t a[8];
  uint32_t b[8];
  for (int i = 0; i < 8; ++i) {
    a[i] = (uint64_t)seed * (threadIdx.x + 1 + i * 7919) * 0x9E3779B97F4A7C15ull;
    b[i] = seed * (threadIdx.x + 3 + i * 31);
  }
  for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if constexpr (OP == 0)  // v_lshrrev_b64 by a register amount
          asm("v_lshrrev_b64 %0, %1, %0" : "+v"(a[i]) : "v"(b[(i + 1) & 7]));
        if constexpr (OP == 1)  // v_lshrrev_b64 by an inline constant
          asm("v_lshrrev_b64 %0, 5, %0" : "+v"(a[i]));
        if constexpr (OP == 2)  // v_lshrrev_b32 (VOP2), for reference
          asm("v_lshrrev_b32 %0, %1, %0" : "+v"(b[i]) : "v"(b[(i + 1) & 7]));
        if constexpr (OP == 3)  // v_lshlrev_b64 by a constant
          asm("v_lshlrev_b64 %0, 3, %0" : "+v"(a[i]));
        if constexpr (OP == 4)  // v_lshl_add_u64
          asm("v_lshl_add_u64 %0, %0, 1, %1" : "+v"(a[i]) : "v"(a[(i + 1) & 7]));
        if constexpr (OP == 5)  // v_mov_b32_dpp wave_shr:1
          asm("v_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(b[i]) : "v"(b[(i + 1) & 7]));
        if constexpr (OP == 6)  // v_bfe_u32 with constant offset/width
          asm("v_bfe_u32 %0, %0, 10, 14" : "+v"(b[i]));
        if constexpr (OP == 7)  // v_and_b32 with a literal
          asm("v_and_b32 %0, 0x1fff8, %0" : "+v"(b[i]));
        if constexpr (OP == 8)  // v_alignbit_b32 with a register amount
          asm("v_alignbit_b32 %0, %1, %0, %2" : "+v"(b[i]) : "v"(b[(i + 1) & 7]), "v"(b[(i + 2) & 7]));
        if constexpr (OP == 9)  // v_pk_mov_b32 (two dwords)
          asm("v_pk_mov_b32 %0, %1, %0 op_sel:[1,0]" : "+v"(a[i]) : "v"(a[(i + 1) & 7]));
      }
    }
  }
  uint32_t s = 0;
  for (int i = 0; i < 8; ++i) s ^= (uint32_t)a[i] ^ (uint32_t)(a[i] >> 32) ^ b[i];
  if (s == 0x12345678) out[0] = s;
}

template <int OP>
double run(uint32_t* out, int grid, uint32_t iters) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipLaunchKernelGGL(k<OP>, dim3(grid), dim3(1024), 0, 0, out, iters, 3u);
  hipEventRecord(e0);
  hipLaunchKernelGGL(k<OP>, dim3(grid), dim3(1024), 0, 0, out, iters, 3u);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  return ms;
}

// The forms stage 1 of the scan kernel chooses between (kernels.hip left_shifts,
// right_shifts, pair_block_addr): cycles of the SIMD's VALU per wave-instruction,
// from the wave's own s_memtime stamps (tick = shader cycle, so the figure
// does not depend on the clock the chip happens to run at).  Four independent
// chains per wave, one 1024-thread workgroup per CU (the 96 KiB of dynamic LDS
// keep a second one off it) = 4 waves per SIMD, one form per kernel.
template <int OP>
__global__ __launch_bounds__(1024) void k4(uint64_t* ticks, uint32_t iters, uint32_t seed) {
  uint32_t b[4];
  for (int i = 0; i < 4; ++i) b[i] = seed * (threadIdx.x + 3 + i * 31);
  const uint32_t c = seed * 0x9E3779B9u + threadIdx.x;   // amount / second source: not on a chain
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (OP == 0)
          asm volatile("v_lshrrev_b32_e32 %0, %1, %0" : "+v"(b[i]) : "v"(c));
        if constexpr (OP == 1)
          asm volatile("v_lshrrev_b32_sdwa %0, %1, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD"
                       : "+v"(b[i]) : "v"(c));
        if constexpr (OP == 2)
          asm volatile("v_alignbit_b32 %0, %1, %0, 23" : "+v"(b[i]) : "v"(c));
        if constexpr (OP == 3)
          asm volatile("v_alignbyte_b32 %0, %1, %0, 2" : "+v"(b[i]) : "v"(c));
      }
    }
  }
  asm volatile("" ::"v"(b[0] ^ b[1] ^ b[2] ^ b[3]));
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  if ((threadIdx.x & 63) == 0) ticks[blockIdx.x * 16 + threadIdx.x / 64] = t1 - t0;
}

template <int OP>
double run4(uint64_t* ticks, uint64_t* host, int grid, uint32_t iters) {
  const size_t lds = 96 << 10;
  if (hipFuncSetAttribute((const void*)k4<OP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -1.0;
  for (int rep = 0; rep < 3; ++rep)   // (the last launch is the one read back)
    hipLaunchKernelGGL(k4<OP>, dim3(grid), dim3(1024), lds, 0, ticks, iters, 3u);
  if (hipMemcpy(host, ticks, sizeof(uint64_t) * grid * 16, hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
  // median over the waves / (4 waves per SIMD x instructions per wave)
  int n = grid * 16;
  for (int i = 1; i < n; ++i)
    for (int j = i; j > 0 && host[j - 1] > host[j]; --j) {
      uint64_t t = host[j];
      host[j] = host[j - 1];
      host[j - 1] = t;
    }
  return (double)host[n / 2] / (4.0 * 64.0 * iters);
}

int stage1_forms(int cus) {
  uint64_t *ticks, *host = new uint64_t[cus * 16];
  if (hipMalloc(&ticks, sizeof(uint64_t) * cus * 16) != hipSuccess) return 1;
  const uint32_t iters = 2048;
  const double c[4] = {run4<0>(ticks, host, cus, iters), run4<1>(ticks, host, cus, iters),
                       run4<2>(ticks, host, cus, iters), run4<3>(ticks, host, cus, iters)};
  const char* names[4] = {"v_lshrrev_b32_e32", "v_lshrrev_b32_sdwa src0_sel:WORD_1", "v_alignbit_b32",
                          "v_alignbyte_b32"};
  printf("{\"what\": \"SIMD cycles per wave-instruction, 4 chains x 4 waves per SIMD\", \"cases\": {");
  for (int o = 0; o < 4; ++o) printf("%s\"%s\": %.3f", o ? ", " : "", names[o], c[o]);
  printf("}}\n");
  hipFree(ticks);
  delete[] host;
  return 0;
}

int main(int argc, char** argv) {
  uint32_t* out;
  hipMalloc(&out, 4);
  int cus;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  if (argc > 1 && argv[1][0] == 's') return stage1_forms(cus);   // valu_rate64 stage1
  const uint32_t iters = 4096;
  const char* names[] = {"lshrrev_b64_v", "lshrrev_b64_k", "lshrrev_b32", "lshlrev_b64_k", "lshl_add_u64",
                         "mov_dpp_wshr", "bfe_k", "and_literal", "alignbit_v", "pk_mov_b32"};
  for (int g : {cus, 2 * cus}) {
    double ms[10] = {run<0>(out, g, iters), run<1>(out, g, iters), run<2>(out, g, iters),
                     run<3>(out, g, iters), run<4>(out, g, iters), run<5>(out, g, iters),
                     run<6>(out, g, iters), run<7>(out, g, iters), run<8>(out, g, iters),
                     run<9>(out, g, iters)};
    for (int o = 0; o < 10; ++o) {
      double winstr = (double)g * 16 * iters * 64;
      printf("grid %d  %-15s %8.3f ms  %.3f wave-instr/clk/CU @2.4GHz\n", g, names[o], ms[o],
             winstr / (ms[o] * 1e-3) / cus / 2.4e9);
    }
  }
  return 0;
}
