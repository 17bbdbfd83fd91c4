// libqmle_sv, Gram matrices of resident states: G[g][r][s] = sum_k conj(a[g][r][k]) b[g][s][k] for groups
// of rows (qmle_gram, qmle_gram_f64).  The device work of the quantum geometric tensor (Script /
// Model quantum_fisher_information): the rows are the unshifted and the shifted circuits of one
// parameter point, Gamma = S^H S is folded with the shift-rule coefficients on the host.
//
// complex64 rows -> v_mfma_f32_32x32x2_f32.  A complex row of length d is a real row of length 2d:
//   Re G[r][s] = sum_x A_r[x] B_s[x],   Im G[r][s] = sum_x A_r[x] B'_s[x],
// B' = B with every (re, im) pair turned into (im, -re) in registers.  A wave owns a 32 x 32 output
// sub-tile (two accumulators: Re and Im), a workgroup of 4 waves a 64 x 64 tile.  The reduction over
// k runs in sub-slices of kGramSub complex amplitudes: 32 chained MFMAs per accumulator element (the MFMA
// is an ordered f32 fma chain; on the diagonal, where every product is positive, a 512-long chain already
// drifts past 1e-6 sum|ab|), each sub-slice added into fp64 registers.  Long rows are cut into
// chunks (one workgroup per output tile x chunk); the chunks' fp64 partials are added by k_gram_reduce
// in chunk order.  Nothing is summed in arrival order: two calls give the same bits.
//
// complex128 rows -> plain fp64 FMA (a 32 x 32 tile per workgroup, 2 x 2 outputs per thread, rows staged
// through LDS), same chunking and the same reduction kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "qmle_internal.h"
#include "qmle_dev.h"

namespace {

constexpr int kGramTile = 64;        // output tile of the complex64 kernel (rows of A x rows of B)
constexpr int kGramSub = 32;         // complex amplitudes per f32 MFMA sub-slice (2 wave iterations)
constexpr int kGramStep = 16;        // complex amplitudes per row per wave iteration (2 halves x 8)
constexpr int kGramTile64 = 32;      // output tile of the complex128 kernel
constexpr int kGramK64 = 32;         // complex128 amplitudes per LDS stage
constexpr int kGramMaxRows = 4096;
constexpr int64_t kGramTargetBlocks = 2048;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GramLayout {
  int tile, nta, ntb, n_pairs, n_chunks;
  int64_t chunk_len;  // complex amplitudes per chunk
  size_t ws_bytes;
};

// Tiles, output-tile pairs, chunks and workspace of one call -- the same numbers on both sides of the
// *_workspace_bytes query.
GramLayout gram_layout(int n_qubits, int n_groups, int rows_a, int rows_b, bool herm, bool f64) {
  GramLayout L{};
  L.tile = f64 ? kGramTile64 : kGramTile;
  L.nta = (rows_a + L.tile - 1) / L.tile;
  L.ntb = (rows_b + L.tile - 1) / L.tile;
  L.n_pairs = herm ? L.nta * (L.nta + 1) / 2 : L.nta * L.ntb;
  const int64_t d = (int64_t)1 << n_qubits;
  const int64_t gran = f64 ? kGramK64 : kGramSub;
  const int64_t max_chunks = (d + gran - 1) / gran;
  const int64_t base = (int64_t)L.n_pairs * n_groups;
  int64_t want = (kGramTargetBlocks + base - 1) / base;
  if (want > max_chunks) want = max_chunks;
  if (want < 1) want = 1;
  int64_t per = (d + want - 1) / want;
  per = (per + gran - 1) / gran * gran;
  if (per > d) per = d;
  L.chunk_len = per;
  L.n_chunks = (int)((d + per - 1) / per);
  L.ws_bytes = L.n_chunks > 1 ? (size_t)n_groups * L.n_pairs * L.n_chunks * L.tile * L.tile * 16 : 0;
  return L;
}

__device__ __forceinline__ void gram_pair(int p, int herm, int nta, int ntb, int &ti, int &tj) {
  if (!herm) {
    ti = p / ntb;
    tj = p - ti * ntb;
    return;
  }
  ti = 0;
  while (p >= nta - ti) {
    p -= nta - ti;
    ++ti;
  }
  tj = ti + p;
}

__device__ __forceinline__ int gram_pair_index(int herm, int nta, int ntb, int ti, int tj) {
  return herm ? ti * nta - ti * (ti - 1) / 2 + (tj - ti) : ti * ntb + tj;
}

// Element (i, j) of the result: direct store (one chunk) with the Hermitian mirror, or the chunk's partial.
__device__ __forceinline__ void gram_put(double2 *__restrict__ out, double2 *__restrict__ part, int herm,
                                         int rows_a, int rows_b, int g, int i, int j, int il, int jl,
                                         int tile, size_t part_base, double re, double im) {
  if (part) {
    part[part_base + (size_t)il * tile + jl] = make_double2(re, im);
    return;
  }
  if (i >= rows_a || j >= rows_b) return;
  double2 *o = out + (size_t)g * rows_a * rows_b;
  if (!herm) {
    o[(size_t)i * rows_b + j] = make_double2(re, im);
    return;
  }
  if (j < i) return;
  if (j == i) {
    o[(size_t)i * rows_b + i] = make_double2(re, 0.0);
    return;
  }
  o[(size_t)i * rows_b + j] = make_double2(re, im);
  o[(size_t)j * rows_b + i] = make_double2(re, -im);
}

// 8 complex64 amplitudes of one row starting at k (zeros past kend; kend - k is even, k is a multiple of 8)
__device__ __forceinline__ void gram_load8(const float4 *__restrict__ row2, int64_t k, int64_t kend,
                                           float4 (&v)[4]) {
  const float4 *p = row2 + (k >> 1);
  if (k + 8 <= kend) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = p[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (k + 2 * j < kend) ? p[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// grid (n_chunks * n_pairs, n_groups), 256 threads.  Block x = chunk * n_pairs + pair (the pairs of one
// chunk are neighbours in dispatch order: they read the same slice of every row).
__global__ void __launch_bounds__(256)
k_gram_f32(const float2 *__restrict__ a, const float2 *__restrict__ b, int64_t d, int rows_a, int rows_b,
           int64_t stride_a, int64_t stride_b, int herm, int nta, int ntb, int n_pairs, int n_chunks,
           int64_t chunk_len, double2 *__restrict__ out, double2 *__restrict__ part) {
  const int g = blockIdx.y;
  const int pair = blockIdx.x % n_pairs, chunk = blockIdx.x / n_pairs;
  int ti, tj;
  gram_pair(pair, herm, nta, ntb, ti, tj);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wy = wave >> 1, wx = wave & 1;
  if (herm && ti == tj && wy > wx) return;  // strictly below the diagonal: the mirror supplies it
  const int r = lane & 31, h = lane >> 5;
  int ra = ti * kGramTile + wy * 32 + r, rb = tj * kGramTile + wx * 32 + r;
  ra = ra < rows_a ? ra : rows_a - 1;  // padding rows read a real row; their results are never stored
  rb = rb < rows_b ? rb : rows_b - 1;
  const float4 *pa = (const float4 *)(a + g * stride_a + (int64_t)ra * d);
  const float4 *pb = (const float4 *)(b + g * stride_b + (int64_t)rb * d);
  const int64_t k0 = (int64_t)chunk * chunk_len;
  const int64_t kend = k0 + chunk_len < d ? k0 + chunk_len : d;

  double dre[16], dim[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) dre[q] = dim[q] = 0.0;
  for (int64_t s0 = k0; s0 < kend; s0 += kGramSub) {
    const int64_t s1 = s0 + kGramSub < kend ? s0 + kGramSub : kend;
    f32x16 cre = {}, cim = {};
    for (int64_t k = s0; k < s1; k += kGramStep) {
      float4 av[4], bv[4];
      const int64_t kk = k + 8 * h;
      gram_load8(pa, kk, s1, av);
      gram_load8(pb, kk, s1, bv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cre = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].x, bv[j].x, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].x, bv[j].y, cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].y, bv[j].y, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].y, -bv[j].x, cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].z, bv[j].z, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].z, bv[j].w, cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].w, bv[j].w, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].w, -bv[j].z, cim, 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      dre[q] += (double)cre[q];
      dim[q] += (double)cim[q];
    }
  }
  const size_t part_base =
      part ? (((size_t)g * n_pairs + pair) * n_chunks + chunk) * kGramTile * kGramTile : 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {  // C/D map of the 32x32 MFMA: col = lane & 31, row = (q&3) + 8(q>>2) + 4(lane>>5)
    const int il = wy * 32 + (q & 3) + 8 * (q >> 2) + 4 * h, jl = wx * 32 + r;
    gram_put(out, part, herm, rows_a, rows_b, g, ti * kGramTile + il, tj * kGramTile + jl, il, jl, kGramTile,
             part_base, dre[q], dim[q]);
  }
}

// complex128: grid (n_chunks * n_pairs, n_groups), 256 threads as 16 x 16, 2 x 2 outputs each.
__global__ void __launch_bounds__(256)
k_gram_f64(const double2 *__restrict__ a, const double2 *__restrict__ b, int64_t d, int rows_a, int rows_b,
           int64_t stride_a, int64_t stride_b, int herm, int nta, int ntb, int n_pairs, int n_chunks,
           int64_t chunk_len, double2 *__restrict__ out, double2 *__restrict__ part) {
  __shared__ double2 sa[kGramTile64][kGramK64 + 1];
  __shared__ double2 sb[kGramTile64][kGramK64 + 1];
  const int g = blockIdx.y;
  const int pair = blockIdx.x % n_pairs, chunk = blockIdx.x / n_pairs;
  int ti, tj;
  gram_pair(pair, herm, nta, ntb, ti, tj);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t k0 = (int64_t)chunk * chunk_len;
  const int64_t kend = k0 + chunk_len < d ? k0 + chunk_len : d;
  const double2 *ga = a + g * stride_a, *gb = b + g * stride_b;
  double acc[2][2][2] = {};
  for (int64_t k = k0; k < kend; k += kGramK64) {
#pragma unroll
    for (int e = 0; e < kGramTile64 * kGramK64 / 256; ++e) {
      const int idx = e * 256 + threadIdx.x;
      const int row = idx / kGramK64, col = idx % kGramK64;
      int ra = ti * kGramTile64 + row, rb = tj * kGramTile64 + row;
      ra = ra < rows_a ? ra : rows_a - 1;
      rb = rb < rows_b ? rb : rows_b - 1;
      const bool in = k + col < kend;
      sa[row][col] = in ? ga[(int64_t)ra * d + k + col] : make_double2(0.0, 0.0);
      sb[row][col] = in ? gb[(int64_t)rb * d + k + col] : make_double2(0.0, 0.0);
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < kGramK64; ++c) {
      const double2 x0 = sa[ty][c], x1 = sa[ty + 16][c];
      const double2 y0 = sb[tx][c], y1 = sb[tx + 16][c];
      const double2 xs[2] = {x0, x1}, ys[2] = {y0, y1};
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          acc[u][v][0] = fma(xs[u].x, ys[v].x, fma(xs[u].y, ys[v].y, acc[u][v][0]));
          acc[u][v][1] = fma(xs[u].x, ys[v].y, fma(-xs[u].y, ys[v].x, acc[u][v][1]));
        }
    }
    __syncthreads();
  }
  const size_t part_base =
      part ? (((size_t)g * n_pairs + pair) * n_chunks + chunk) * kGramTile64 * kGramTile64 : 0;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int il = ty + 16 * u, jl = tx + 16 * v;
      gram_put(out, part, herm, rows_a, rows_b, g, ti * kGramTile64 + il, tj * kGramTile64 + jl, il, jl,
               kGramTile64, part_base, acc[u][v][0], acc[u][v][1]);
    }
}

// Sum of the chunk partials in chunk order (fp64), Hermitian mirror; one thread per output element.
__global__ void __launch_bounds__(256)
k_gram_reduce(const double2 *__restrict__ part, int n_groups, int rows_a, int rows_b, int herm, int tile,
              int nta, int ntb, int n_pairs, int n_chunks, double2 *__restrict__ out) {
  const int64_t per = (int64_t)rows_a * rows_b;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= per * n_groups) return;
  const int g = (int)(idx / per);
  const int64_t e = idx - (int64_t)g * per;
  int i = (int)(e / rows_b), j = (int)(e - (int64_t)i * rows_b);
  const bool mirror = herm && j < i;
  if (mirror) {
    const int t = i;
    i = j;
    j = t;
  }
  const int ti = i / tile, tj = j / tile, il = i - ti * tile, jl = j - tj * tile;
  const int p = gram_pair_index(herm, nta, ntb, ti, tj);
  const double2 *src = part + ((size_t)g * n_pairs + p) * n_chunks * tile * tile + (size_t)il * tile + jl;
  double re = 0.0, im = 0.0;
  for (int c = 0; c < n_chunks; ++c) {
    const double2 v = src[(size_t)c * tile * tile];
    re += v.x;
    im += v.y;
  }
  if (herm && i == j) im = 0.0;
  out[idx] = make_double2(re, mirror ? -im : im);
}

int gram_run(const void *d_a, const void *d_b, int n_qubits, int n_groups, int rows_a, int rows_b,
             int64_t group_stride_a, int64_t group_stride_b, void *d_out, void *d_ws, size_t ws_bytes,
             qmle_stream stream_, bool f64) {
  if (!d_a || !d_b || !d_out || n_qubits < 1 || n_qubits > 30 || n_groups < 1 ||
      n_groups > kMaxGridY || rows_a < 1 || rows_b < 1 || rows_a > kGramMaxRows ||
      rows_b > kGramMaxRows || group_stride_a < 0 || group_stride_b < 0)
    return QMLE_ERR_INVALID_ARG;
  const int64_t d = (int64_t)1 << n_qubits;
  // (complex64 rows are read as float4 pairs: every row must start on an even amplitude)
  if (!f64 && (((uintptr_t)d_a | (uintptr_t)d_b) % 16 != 0 || (group_stride_a | group_stride_b) % 2 != 0))
    return QMLE_ERR_INVALID_ARG;
  if (n_groups > 1 && (group_stride_a < (int64_t)rows_a * d || group_stride_b < (int64_t)rows_b * d))
    return QMLE_ERR_INVALID_ARG;
  if ((int64_t)n_groups * rows_a * rows_b > ((int64_t)1 << 39)) return QMLE_ERR_INVALID_ARG;  // reduce grid
  const bool herm = d_a == d_b && rows_a == rows_b && group_stride_a == group_stride_b;
  const GramLayout L = gram_layout(n_qubits, n_groups, rows_a, rows_b, herm, f64);
  if (L.ws_bytes && (!d_ws || ws_bytes < L.ws_bytes)) return QMLE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  double2 *part = L.n_chunks > 1 ? (double2 *)d_ws : nullptr;
  const dim3 grid((unsigned)((int64_t)L.n_chunks * L.n_pairs), (unsigned)n_groups);
  if (f64)
    hipLaunchKernelGGL(k_gram_f64, grid, dim3(256), 0, stream, (const double2 *)d_a, (const double2 *)d_b, d,
                       rows_a, rows_b, group_stride_a, group_stride_b, (int)herm, L.nta, L.ntb, L.n_pairs,
                       L.n_chunks, L.chunk_len, (double2 *)d_out, part);
  else
    hipLaunchKernelGGL(k_gram_f32, grid, dim3(256), 0, stream, (const float2 *)d_a, (const float2 *)d_b, d,
                       rows_a, rows_b, group_stride_a, group_stride_b, (int)herm, L.nta, L.ntb, L.n_pairs,
                       L.n_chunks, L.chunk_len, (double2 *)d_out, part);
  HIPCHK(hipGetLastError());
  if (part) {
    const int64_t total = (int64_t)n_groups * rows_a * rows_b;
    hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       (const double2 *)part, n_groups, rows_a, rows_b, (int)herm, L.tile, L.nta, L.ntb,
                       L.n_pairs, L.n_chunks, (double2 *)d_out);
    HIPCHK(hipGetLastError());
  }
  return QMLE_OK;
}

size_t gram_ws(int n_qubits, int n_groups, int rows_a, int rows_b, bool f64) {
  if (n_qubits < 1 || n_qubits > 30 || n_groups < 1 || rows_a < 1 || rows_b < 1) return 0;
  // the larger of the Hermitian and the general layout: the query does not know whether A == B
  const GramLayout h = gram_layout(n_qubits, n_groups, rows_a, rows_b, rows_a == rows_b, f64);
  const GramLayout g = gram_layout(n_qubits, n_groups, rows_a, rows_b, false, f64);
  return h.ws_bytes > g.ws_bytes ? h.ws_bytes : g.ws_bytes;
}

}  // namespace

extern "C" {

int qmle_gram(const void *d_a, const void *d_b, int n_qubits, int n_groups, int rows_a, int rows_b,
              int64_t group_stride_a, int64_t group_stride_b, void *d_out, void *d_ws, size_t ws_bytes,
              qmle_stream stream) {
  return gram_run(d_a, d_b, n_qubits, n_groups, rows_a, rows_b, group_stride_a, group_stride_b, d_out, d_ws,
                  ws_bytes, stream, false);
}

size_t qmle_gram_workspace_bytes(int n_qubits, int n_groups, int rows_a, int rows_b) {
  return gram_ws(n_qubits, n_groups, rows_a, rows_b, false);
}

int qmle_gram_f64(const void *d_a, const void *d_b, int n_qubits, int n_groups, int rows_a, int rows_b,
                  int64_t group_stride_a, int64_t group_stride_b, void *d_out, void *d_ws, size_t ws_bytes,
                  qmle_stream stream) {
  return gram_run(d_a, d_b, n_qubits, n_groups, rows_a, rows_b, group_stride_a, group_stride_b, d_out, d_ws,
                  ws_bytes, stream, true);
}

size_t qmle_gram_workspace_bytes_f64(int n_qubits, int n_groups, int rows_a, int rows_b) {
  return gram_ws(n_qubits, n_groups, rows_a, rows_b, true);
}

}  // extern "C"
