// libqmle_sv, the matrix cotangent of a dense gate on three or four wires (qmle_wide_moment): the moment
// M[a][c] = sum_rest conj(lambda[a, rest]) psi[c, rest] of two resident states as a small GEMM on the matrix cores,
// per-block partial sums in the caller's workspace, and one finishing kernel that adds them in double and applies
// (U^+)^T (cot_finish_entry of qmle_adjoint_dev.h).  Both precisions, one read of psi and of lambda, no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "qmle_internal.h"
#include "qmle_host.h"
#include "qmle_dev.h"
#include "qmle_adjoint_dev.h"

namespace {

typedef float wide_f4 __attribute__((ext_vector_type(4)));
typedef double wide_d4 __attribute__((ext_vector_type(4)));

constexpr int kWideGroupsPerLane = 4;   // groups a lane loads per iteration: four contraction steps
constexpr int kWideIterations = 8;      // iterations per wave a launch is sized for (two per trip of the loop)
constexpr int kWideMaxBlocks = 1024;    // blocks per state

struct WideWires {
  int sp[4];   // the targets' bit positions, ascending
  int bpos[4]; // bit q of the caller's matrix index sits on position bpos[q]
};

// four consecutive amplitudes: two 16-byte loads in complex64 (the caller guarantees 32-byte alignment)
__device__ __forceinline__ void wide_load4(const float2 *__restrict__ p, float2 (&v)[4]) {
  const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
  v[0] = make_float2(a.x, a.y), v[1] = make_float2(a.z, a.w), v[2] = make_float2(b.x, b.y), v[3] = make_float2(b.z, b.w);
}
__device__ __forceinline__ void wide_load4(const double2 *__restrict__ p, double2 (&v)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = p[j];
}
// D += A B for A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
__device__ __forceinline__ wide_f4 wide_mfma(float a, float b, wide_f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ wide_d4 wide_mfma(double a, double b, wide_d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// partial[sample][block][a * D + c] = sum over the block's groups of conj(lambda[a, group]) psi[c, group], a and c in
// the caller's matrix order.  A team of D lanes holds the D amplitudes of one group, so a wave holds 64 / D groups per
// contraction step: at D = 16 they are the four k-slots of one 16x16x4 instruction; at D = 8 two groups sit side by
// side in the 16 rows and columns, and only the two diagonal 8x8 blocks of the product are kept.  Re and Im of the
// moment are two accumulators fed by four instructions per step.  Which group a team takes is free (the contraction
// sums them all), so a lane takes kWideGroupsPerLane CONSECUTIVE groups: with no target below position 2 (CONTIG) they
// are 32 (64) contiguous bytes, and the four teams of a row together read whole 128-byte lines.  Groups past the end
// of the state (n - K < 4 or so) are zeros, never read.  Control flow around the matrix instructions is wave-uniform.
template <int K, bool F64, bool CONTIG>
__global__ void __launch_bounds__(256)
k_wide_moment(const void *__restrict__ psi_all, const void *__restrict__ lam_all, int n, const WideWires W,
              void *__restrict__ partial_all) {
  constexpr int D = 1 << K, TEAMS = kWave / D, GPL = kWideGroupsPerLane;
  using V = std::conditional_t<F64, double2, float2>;
  using T = std::conditional_t<F64, double, float>;
  using ACC = std::conditional_t<F64, wide_d4, wide_f4>;
  __shared__ T red[4][256][2];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int amp = lane & (D - 1), team = lane / D;
  uint64_t off = 0;
#pragma unroll
  for (int q = 0; q < K; ++q) off |= (uint64_t)((amp >> q) & 1) << W.bpos[q];
  off += (uint64_t)blockIdx.y << n;
  const V *__restrict__ psi = (const V *)psi_all + off, *__restrict__ lam = (const V *)lam_all + off;
  const uint64_t groups = (uint64_t)1 << (n - K);
  const uint64_t per_wave = (uint64_t)TEAMS * GPL, stride = (uint64_t)gridDim.x * 4u * per_wave;
  ACC re = {0, 0, 0, 0}, im = {0, 0, 0, 0};
  // two wave-iterations per trip: the loads of both are issued ahead of their matrix instructions
  for (uint64_t gw = ((uint64_t)blockIdx.x * 4u + wv) * per_wave; gw < groups; gw += 2 * stride) {  // (wave-uniform)
    V p[2][GPL], l[2][GPL];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint64_t g0 = gw + (uint64_t)h * stride + (uint64_t)team * GPL;
#pragma unroll
      for (int j = 0; j < GPL; ++j) p[h][j] = V{0, 0}, l[h][j] = V{0, 0};
      if constexpr (CONTIG) {  // groups a multiple of GPL, sp[0] >= 2: the low two bits of g0 pass through the inserts
        if (g0 < groups) {
          uint64_t base = g0;
#pragma unroll
          for (int q = 0; q < K; ++q) base = ins0_64(base, W.sp[q]);
          wide_load4(psi + base, p[h]);
          wide_load4(lam + base, l[h]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < GPL; ++j)
          if (g0 + j < groups) {
            uint64_t base = g0 + j;
#pragma unroll
            for (int q = 0; q < K; ++q) base = ins0_64(base, W.sp[q]);
            p[h][j] = psi[base];
            l[h][j] = lam[base];
          }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < GPL; ++j) {  // conj(l) p = (l.x p.x + l.y p.y) + i (l.x p.y - l.y p.x)
        re = wide_mfma(l[h][j].x, p[h][j].x, re);
        im = wide_mfma(l[h][j].x, p[h][j].y, im);
        re = wide_mfma(l[h][j].y, p[h][j].y, re);
        im = wide_mfma(-l[h][j].y, p[h][j].x, im);
      }
  }
  // the accumulators' (row, column): column = lane & 15; row = 4 (lane >> 4) + r in float32, (lane >> 4) + 4 r in float64
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = F64 ? (lane >> 4) + 4 * r : 4 * (lane >> 4) + r;
    red[wv][row * 16 + (lane & 15)][0] = re[r];
    red[wv][row * 16 + (lane & 15)][1] = im[r];
  }
  __syncthreads();
  if (threadIdx.x < D * D) {
    const int a = threadIdx.x / D, c = threadIdx.x % D;
    T sr = 0, si = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int h = 0; h < 16 / D; ++h) {  // (D = 8: the two diagonal blocks)
        sr += red[w][(a + h * D) * 16 + c + h * D][0];
        si += red[w][(a + h * D) * 16 + c + h * D][1];
      }
    V v;
    v.x = sr, v.y = si;
    ((V *)partial_all)[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (D * D) + threadIdx.x] = v;
  }
}

// cot[sample] = (sum_blocks partial[sample][block]) (U^+)^T, summed in double in a fixed order; U the FORWARD matrix
// of the sample in the caller's wire order, or none (mats == nullptr): the moment itself.  One block of 1024 threads
// per sample: 1024 / D^2 threads share an entry, each sums every (1024 / D^2)-th block (a thread alone would wait for
// up to 1024 dependent loads, a quarter of a millisecond), and their sums are added in thread order.
template <int K, class V, class OT>
__global__ void __launch_bounds__(1024)
k_wide_moment_finish(const V *__restrict__ partial, int n_blocks, const double2 *__restrict__ mats, int per_sample,
                     OT *__restrict__ cot) {
  constexpr int D = 1 << K, DD = D * D, PARTS = 1024 / DD;
  __shared__ double part[PARTS][DD * 2], m[DD * 2], ud[DD * 2];
  const int b = blockIdx.x, t = threadIdx.x % DD, p = threadIdx.x / DD;
  const double2 *__restrict__ u = mats ? mats + (per_sample ? (size_t)b * DD : 0) : nullptr;
  double sr = 0.0, si = 0.0;
#pragma unroll 4
  for (int k = p; k < n_blocks; k += PARTS) {
    const V v = partial[((size_t)b * n_blocks + k) * DD + t];
    sr += v.x;
    si += v.y;
  }
  part[p][2 * t] = sr, part[p][2 * t + 1] = si;
  __syncthreads();
  if (p == 0) {
    sr = 0.0, si = 0.0;
#pragma unroll
    for (int q = 0; q < PARTS; ++q) sr += part[q][2 * t], si += part[q][2 * t + 1];
    m[2 * t] = sr, m[2 * t + 1] = si;
    if (u) {  // U^+[c][d] = conj(U[d][c])
      const double2 e = u[(t % D) * D + t / D];
      ud[2 * t] = e.x, ud[2 * t + 1] = -e.y;
    }
  }
  __syncthreads();
  if (p == 0) {
    double gr = m[2 * t], gi = m[2 * t + 1];
    if (u) cot_finish_entry<D>((const double *)m, (const double *)ud, t / D, t % D, gr, gi);
    cot[((size_t)b * DD + t) * 2] = (OT)gr;
    cot[((size_t)b * DD + t) * 2 + 1] = (OT)gi;
  }
}

int wide_blocks(int n, int k) {
  const uint64_t groups = (uint64_t)1 << (n - k);
  const uint64_t per_block = (uint64_t)4 * (kWave >> k) * kWideGroupsPerLane * kWideIterations;
  return (int)std::min<uint64_t>(std::max<uint64_t>((groups + per_block - 1) / per_block, 1), kWideMaxBlocks);
}
size_t wide_ws_bytes(int n, int batch, int k, int f64) {
  const size_t in_flight = (size_t)std::min(batch, kMaxGridY);
  return in_flight * wide_blocks(n, k) * ((size_t)1 << (2 * k)) * (f64 ? sizeof(double2) : sizeof(float2)) + 256;
}

template <int K, bool F64>
void wide_launch(bool contig, dim3 grid, hipStream_t stream, const void *psi, const void *lam, int n, const WideWires &W,
                 void *partial, int nb, const double2 *mats, int per_sample, void *cot) {
  using V = std::conditional_t<F64, double2, float2>;
  using OT = std::conditional_t<F64, double, float>;
  if (contig) hipLaunchKernelGGL((k_wide_moment<K, F64, true>), grid, dim3(256), 0, stream, psi, lam, n, W, partial);
  else hipLaunchKernelGGL((k_wide_moment<K, F64, false>), grid, dim3(256), 0, stream, psi, lam, n, W, partial);
  hipLaunchKernelGGL((k_wide_moment_finish<K, V, OT>), dim3(grid.y), dim3(1024), 0, stream, (const V *)partial, nb, mats,
                     per_sample, (OT *)cot);
}

}  // namespace

extern "C" {

size_t qmle_wide_moment_workspace_bytes(int n_qubits, int batch, int k, int f64) {
  if ((k != 3 && k != 4) || batch < 1 || n_qubits < k || n_qubits > QMLE_MAX_QUBITS || (f64 != 0 && f64 != 1)) return 0;
  return wide_ws_bytes(n_qubits, batch, k, f64);
}

int qmle_wide_moment(const void *d_psi, const void *d_lam, int n_qubits, int batch, int f64, const int32_t *wires, int k,
                     const void *d_mats, int per_sample, void *d_cot, void *d_ws, size_t ws_bytes, qmle_stream stream_) {
  if (k != 3 && k != 4) return QMLE_ERR_UNSUPPORTED;
  if (!d_psi || !d_lam || !wires || !d_cot || !d_ws || batch < 1 || n_qubits < k || n_qubits > QMLE_MAX_QUBITS ||
      (f64 != 0 && f64 != 1) || (per_sample != 0 && per_sample != 1))
    return QMLE_ERR_INVALID_ARG;
  for (int i = 0; i < k; ++i)
    if (wires[i] < 0 || wires[i] >= n_qubits) return QMLE_ERR_WIRE_RANGE;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < i; ++j)
      if (wires[i] == wires[j]) return QMLE_ERR_DUPLICATE_WIRES;
  const int n = n_qubits;
  char *ws = (char *)d_ws;  // (the query's answer holds 256 bytes for aligning it)
  if (ws_bytes < wide_ws_bytes(n, batch, k, f64) || !align_workspace(ws, ws_bytes)) return QMLE_ERR_WORKSPACE;
  // wire i is bit k - 1 - i of the matrix index (the first wire the most significant) and sits on position n - 1 - wire
  WideWires W{};
  for (int i = 0; i < k; ++i) W.bpos[k - 1 - i] = W.sp[i] = n - 1 - wires[i];
  std::sort(W.sp, W.sp + k);
  const bool contig = W.sp[0] >= 2;
  const int nb = wide_blocks(n, k);
  const size_t amp = f64 ? sizeof(double2) : sizeof(float2), dd = (size_t)1 << (2 * k);
  hipStream_t stream = (hipStream_t)stream_;
  for (int b0 = 0; b0 < batch; b0 += kMaxGridY) {
    const int nbatch = std::min(kMaxGridY, batch - b0);
    const char *psi = (const char *)d_psi + ((size_t)b0 << n) * amp, *lam = (const char *)d_lam + ((size_t)b0 << n) * amp;
    const double2 *mats = d_mats ? (const double2 *)d_mats + (per_sample ? (size_t)b0 * dd : 0) : nullptr;
    char *cot = (char *)d_cot + (size_t)b0 * dd * amp;
    const dim3 grid((unsigned)nb, (unsigned)nbatch);
    if (k == 3) {
      if (f64) wide_launch<3, true>(contig, grid, stream, psi, lam, n, W, ws, nb, mats, per_sample, cot);
      else wide_launch<3, false>(contig, grid, stream, psi, lam, n, W, ws, nb, mats, per_sample, cot);
    } else {
      if (f64) wide_launch<4, true>(contig, grid, stream, psi, lam, n, W, ws, nb, mats, per_sample, cot);
      else wide_launch<4, false>(contig, grid, stream, psi, lam, n, W, ws, nb, mats, per_sample, cot);
    }
    HIPCHK(hipGetLastError());
  }
  return QMLE_OK;
}

}  // extern "C"
