// What the measuring walk pays to hand 16 amplitudes per work item from one gate group's frame to the next (DESIGN
// 4.7, 9k), in isolation, between two dense gates' worth of packed FMAs (2 x 64 v_pk_fma_f32) per round:
//   mode 0  the FMAs alone;
//   mode 1  + 32 lane swaps: in-thread bit 2 <-> lane bit 4 (16 v_permlane16_swap_b32), bit 3 <-> lane bit 5
//           (16 v_permlane32_swap_b32);
//   mode 2  + the transposition through LDS they replace: 16 ds_write_b64, 16 ds_read_b64 of slots other lanes of the
//           same wave wrote (wave-private, no barrier: a wave's LDS operations execute in order), 2 x 16 v_xor for
//           the addresses.
// Five 256-thread workgroups per CU with 32 KiB of LDS each, as the walk runs.  Registers and LDS only, no global
// traffic inside the loop.
//   hipcc -O3 --offload-arch=gfx950 tools/lane_swap_bench.hip -o tools/bin/lane_swap_bench
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float v2f __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

__device__ __forceinline__ void swap16(v2f &a, v2f &b) {
  const auto lo = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
  a = (v2f){__uint_as_float(lo[0]), __uint_as_float(hi[0])};
  b = (v2f){__uint_as_float(lo[1]), __uint_as_float(hi[1])};
}
__device__ __forceinline__ void swap32(v2f &a, v2f &b) {
  const auto lo = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
  a = (v2f){__uint_as_float(lo[0]), __uint_as_float(hi[0])};
  b = (v2f){__uint_as_float(lo[1]), __uint_as_float(hi[1])};
}

template <int MODE>
__global__ void __launch_bounds__(256) k_round(float *out, const float *coef, int iters) {
  extern __shared__ v2f tile[];  // 4096 slots = 32 KiB
  v2f r[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) r[c] = (v2f){1.0f + 0.001f * (float)(threadIdx.x + c), 0.5f};
  const v2f m = (v2f){coef[0], coef[0]}, k = (v2f){coef[1], coef[1]};
  // slot of amplitude c: c << 8 | thread; the gather reads c << 8 | (thread ^ 4 c): another lane of the same wave
  const unsigned wr = threadIdx.x, rd = threadIdx.x;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int rep = 0; rep < 4; ++rep)
#pragma unroll
      for (int c = 0; c < 16; ++c) r[c] = __builtin_elementwise_fma(r[c], m, k);
    if (MODE == 1) {
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (!(c & 4)) swap16(r[c], r[c | 4]);
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (!(c & 8)) swap32(r[c], r[c | 8]);
    }
    if (MODE == 2) {
#pragma unroll
      for (int c = 0; c < 16; ++c) tile[wr ^ (unsigned)(c << 8)] = r[c];
      asm volatile("" ::: "memory");
#pragma unroll
      for (int c = 0; c < 16; ++c) r[c] = tile[rd ^ (unsigned)((c << 8) | ((4 * c) & 63))];
      asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int rep = 0; rep < 4; ++rep)
#pragma unroll
      for (int c = 0; c < 16; ++c) r[c] = __builtin_elementwise_fma(r[c], m, k);
  }
  v2f s = (v2f){0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 16; ++c) s += r[c];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s.x + s.y;
}

int main() {
  float *d, *coef;
  const int blocks = 256 * 5 * 4, iters = 2000;
  if (hipMalloc(&d, (size_t)blocks * 256 * sizeof(float)) != hipSuccess || hipMalloc(&coef, 8) != hipSuccess) return 1;
  const float hc[2] = {0.999f, 0.001f};
  hipMemcpy(coef, hc, 8, hipMemcpyHostToDevice);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  const char *names[3] = {"128 packed FMAs", "128 packed FMAs + 32 lane swaps", "128 packed FMAs + LDS scatter / gather"};
  float best[3];
  for (int mode = 0; mode < 3; ++mode) {
    best[mode] = 1e9f;
    for (int rep = 0; rep < 4; ++rep) {
      hipEventRecord(e0);
      if (mode == 0) hipLaunchKernelGGL(k_round<0>, dim3(blocks), dim3(256), 32768, 0, d, coef, iters);
      if (mode == 1) hipLaunchKernelGGL(k_round<1>, dim3(blocks), dim3(256), 32768, 0, d, coef, iters);
      if (mode == 2) hipLaunchKernelGGL(k_round<2>, dim3(blocks), dim3(256), 32768, 0, d, coef, iters);
      hipEventRecord(e1);
      if (hipEventSynchronize(e1) != hipSuccess) return 1;
      float ms;
      hipEventElapsedTime(&ms, e0, e1);
      if (rep > 0 && ms < best[mode]) best[mode] = ms;  // (the first launch loads the code object)
    }
    // rounds per SIMD: 4 waves per workgroup, 4 SIMDs per CU, 256 CUs
    const double rounds = (double)iters * blocks * 4 / 1024.0;
    printf("%-40s %8.3f ms  %7.1f cycles per round per SIMD at 2.4 GHz", names[mode], best[mode], best[mode] * 1e-3 * 2.4e9 / rounds);
    if (mode) printf("  (+%.1f over the FMAs alone)", (best[mode] - best[0]) * 1e-3 * 2.4e9 / rounds);
    printf("\n");
  }
  return 0;
}
