// libqmle_sv, measurement and analysis kernels of resident states: <Z> / parities, probabilities,
// density matrices, marginals, overlaps and pair fidelities, histogram, the parameter sampler and shot
// sampling -- with their C-ABI entry points.  (Meyer-Wallach: qmle_mw.hip.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <new>
#include <utility>

#include "qmle_internal.h"
#include "qmle_host.h"
#include "qmle_dev.h"

namespace {

// ---------------------------------------------------------------------------
// all-qubit <Z> in one read.  Element index bits: bit0 = position inside the
// float4 chunk, bits 1..8 = thread id, bits 9..10 = unroll slot u, bits >= 11 =
// segment id.  Every bit gets its own signed accumulator (static indexing).
// ---------------------------------------------------------------------------
constexpr int kEzThreads = 256;
constexpr int kEzUnroll = 4;
constexpr int kEzSegBits = 11;  // 1 + 8 + 2
constexpr int kEzMaxHigh = QMLE_MAX_QUBITS - kEzSegBits;

__global__ void __launch_bounds__(kEzThreads)
k_expval_partial(const float4 *__restrict__ states, int n, float *__restrict__ partial) {
  __shared__ float red[16];
  const int b = blockIdx.y, tid = threadIdx.x;
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const float4 *st = states + (size_t)b * chunks;
  const uint64_t seg_chunks = (uint64_t)kEzThreads * kEzUnroll;
  const uint64_t n_seg = (chunks + seg_chunks - 1) / seg_chunks;
  float acc_tot = 0.f, acc_b0 = 0.f, acc_u0 = 0.f, acc_u1 = 0.f;
  float acc_hi[kEzMaxHigh];
#pragma unroll
  for (int k = 0; k < kEzMaxHigh; ++k) acc_hi[k] = 0.f;
  for (uint64_t seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
    float4 v[kEzUnroll];
#pragma unroll
    for (int u = 0; u < kEzUnroll; ++u) {
      const uint64_t c = seg * seg_chunks + (uint64_t)u * kEzThreads + tid;
      v[u] = c < chunks ? st[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float pe = 0.f, po = 0.f, pu[kEzUnroll];
#pragma unroll
    for (int u = 0; u < kEzUnroll; ++u) {
      const float e = v[u].x * v[u].x + v[u].y * v[u].y;
      const float o = v[u].z * v[u].z + v[u].w * v[u].w;
      pe += e;
      po += o;
      pu[u] = e + o;
    }
    const float tot = pe + po;
    acc_tot += tot;
    acc_b0 += pe - po;
    acc_u0 += (pu[0] - pu[1]) + (pu[2] - pu[3]);
    acc_u1 += (pu[0] + pu[1]) - (pu[2] + pu[3]);
#pragma unroll
    for (int k = 0; k < kEzMaxHigh; ++k) acc_hi[k] += ((seg >> k) & 1ull) ? -tot : tot;
  }
  // partial[b][block][bit]; bit n is the plain total (norm check)
  float *out = partial + ((size_t)b * gridDim.x + blockIdx.x) * (QMLE_MAX_QUBITS + 1);
  float r;
  r = block_sum(acc_b0, red);
  if (tid == 0) out[0] = r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    r = block_sum(((tid >> i) & 1) ? -acc_tot : acc_tot, red);
    if (tid == 0) out[1 + i] = r;
  }
  r = block_sum(acc_u0, red);
  if (tid == 0) out[9] = r;
  r = block_sum(acc_u1, red);
  if (tid == 0) out[10] = r;
#pragma unroll
  for (int k = 0; k < kEzMaxHigh; ++k) {
    r = block_sum(acc_hi[k], red);
    if (tid == 0) out[kEzSegBits + k] = r;
  }
  r = block_sum(acc_tot, red);
  if (tid == 0) out[QMLE_MAX_QUBITS] = r;
}


// one block per (state, observable): fp64 sum of that bit's column over all partial rows
__global__ void __launch_bounds__(256)
k_expval_final(const float *__restrict__ partial, int n_blocks, int n_obs, ObsBits obs,
               float *__restrict__ out) {
  __shared__ double red[16];
  const int b = blockIdx.x, k = blockIdx.y;
  const float *pp = partial + (size_t)b * n_blocks * (QMLE_MAX_QUBITS + 1) + obs.bits[k];
  const uint32_t rm = obs.row_mask[k];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_blocks; i += blockDim.x) {
    const double v = (double)pp[(size_t)i * (QMLE_MAX_QUBITS + 1)];
    acc += (__popc(rm & (uint32_t)i) & 1) ? -v : v;
  }
  const double tot = block_sum_d(acc, red);
  if (threadIdx.x == 0) out[(size_t)b * n_obs + k] = (float)tot;
}

// ---------------------------------------------------------------------------
// simple streaming kernels
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_probs(const float4 *__restrict__ states, float2 *__restrict__ out, uint64_t total_chunks) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total_chunks; k += stride) {
    const float4 v = states[k];
    out[k] = make_float2(v.x * v.x + v.y * v.y, v.z * v.z + v.w * v.w);
  }
}

__global__ void __launch_bounds__(256)
k_density(const float2 *__restrict__ states, float2 *__restrict__ out, int n) {
  const int b = blockIdx.y;
  const uint64_t D = (uint64_t)1 << n;
  const float2 *st = states + (size_t)b * D;
  float2 *o = out + (size_t)b * D * D;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < D * D; k += stride) {
    const uint64_t i = k >> n, j = k & (D - 1);
    const float2 a = st[i], c = st[j];
    o[k] = make_float2(a.x * c.x + a.y * c.y, a.y * c.x - a.x * c.y);  // a * conj(c)
  }
}

struct KeepBits {
  int8_t bits[QMLE_MAX_QUBITS];  // bit positions of kept wires, LSB of output first
  int n_keep;
};

// Few kept wires (<= 12): every workgroup bins its share of |a|^2 in LDS first and adds one value
// per bin to the output -- 2^n / grid terms per global atomic instead of one.  (One global float
// atomic per amplitude left partial probabilities 2e-6 .. 2e-5 apart between two runs on the
// same state at n = 18, and it is the slowest way to add.)
__global__ void __launch_bounds__(256)
k_marginal_lds(const float2 *__restrict__ states, float *__restrict__ out, int n, KeepBits kb) {
  extern __shared__ float4 smem4[];
  float *bins = reinterpret_cast<float *>(smem4);
  const int b = blockIdx.y;
  const uint32_t n_bins = 1u << kb.n_keep;
  for (uint32_t k = threadIdx.x; k < n_bins; k += blockDim.x) bins[k] = 0.f;
  __syncthreads();
  const uint64_t D = (uint64_t)1 << n;
  const float2 *st = states + (size_t)b * D;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < D; i += stride) {
    uint32_t idx = 0;
    for (int k = 0; k < kb.n_keep; ++k) idx |= (uint32_t)((i >> kb.bits[k]) & 1ull) << k;
    atomicAdd(bins + idx, norm2(st[i]));
  }
  __syncthreads();
  float *o = out + ((size_t)b << kb.n_keep);
  for (uint32_t k = threadIdx.x; k < n_bins; k += blockDim.x) {
    const float v = bins[k];
    if (v != 0.f) atomicAdd(o + k, v);
  }
}

__global__ void __launch_bounds__(256)
k_marginal(const float2 *__restrict__ states, float *__restrict__ out, int n, KeepBits kb) {
  const int b = blockIdx.y;
  const uint64_t D = (uint64_t)1 << n;
  const float2 *st = states + (size_t)b * D;
  float *o = out + ((size_t)b << kb.n_keep);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < D; i += stride) {
    uint32_t idx = 0;
    for (int k = 0; k < kb.n_keep; ++k) idx |= (uint32_t)((i >> kb.bits[k]) & 1ull) << k;
    atomicAdd(o + idx, norm2(st[i]));
  }
}

// <a|b> partial sums: partial[pair][block] = (re, im)
__global__ void __launch_bounds__(256)
k_overlap_partial(const float4 *__restrict__ states, int n, int n_pairs,
                  float2 *__restrict__ partial) {
  __shared__ float red[16];
  const int pr = blockIdx.y;
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const float4 *a = states + (size_t)pr * chunks;
  const float4 *c = states + ((size_t)pr + n_pairs) * chunks;
  float re = 0.f, im = 0.f;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < chunks; k += stride) {
    const float4 x = a[k], y = c[k];
    // conj(x) * y
    re += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    im += x.x * y.y - x.y * y.x + x.z * y.w - x.w * y.z;
  }
  const float r = block_sum(re, red);
  const float i = block_sum(im, red);
  if (threadIdx.x == 0) partial[(size_t)pr * gridDim.x + blockIdx.x] = make_float2(r, i);
}

__global__ void __launch_bounds__(256)
k_overlap_final(const float2 *__restrict__ partial, int n_blocks, int n_pairs,
                float *__restrict__ out) {
  __shared__ double red[16];
  const int pr = blockIdx.x;
  double re = 0.0, im = 0.0;
  for (int i = threadIdx.x; i < n_blocks; i += blockDim.x) {
    const float2 v = partial[(size_t)pr * n_blocks + i];
    re += v.x;
    im += v.y;
  }
  re = block_sum_d(re, red);
  im = block_sum_d(im, red);
  if (threadIdx.x == 0) out[pr] = (float)(re * re + im * im);
}
// Small states (n <= 16): ONE workgroup per pair, no partial rows -- the two-launch form spent 17 us
// on 1024 pairs of 12-qubit states, most of it launch latency and the row round trip.  fp32 inside a
// thread (<= 128 products each), fp64 across the workgroup.
__global__ void __launch_bounds__(256)
k_pair_fidelity_small(const float4 *__restrict__ states, int n, int n_pairs, float *__restrict__ out) {
  __shared__ double red[16];
  const int pr = blockIdx.x;
  const uint32_t chunks = 1u << (n - 1);
  const float4 *a = states + (size_t)pr * chunks;
  const float4 *c = states + ((size_t)pr + n_pairs) * chunks;
  float re = 0.f, im = 0.f;
  for (uint32_t k = threadIdx.x; k < chunks; k += blockDim.x) {
    const float4 x = a[k], y = c[k];  // conj(x) * y
    re += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    im += x.x * y.y - x.y * y.x + x.z * y.w - x.w * y.z;
  }
  const double r = block_sum_d((double)re, red);
  const double i = block_sum_d((double)im, red);
  if (threadIdx.x == 0) out[pr] = (float)(r * r + i * i);
}

// ---- parameter sampler on the device ---------------------------------------------------------
// numpy's Philox4x64-10 stream (csrc/qmle_rng.cpp restates it on the host): block b of the stream
// is philox(counter = b + 1, key) -- any block on its own, one work item per block of four values.
// The arithmetic after the generator is numpy's, rounding for rounding: u = (x >> 11) * 2^-53
// (exact), low + range * u as a rounded product and a rounded sum (no fused multiply-add), cast to
// float32.  Expressibility(12 q, 1024 pairs) spent 0.4 of its 0.9 ms drawing parameters on the host.
__device__ __forceinline__ void philox_uniform_body(uint64_t k0, uint64_t k1, uint64_t n, double low, double range,
                                                    float *__restrict__ out) {
  const uint64_t blocks = (n + 3) / 4;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks; b += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t c0 = b + 1, c1 = 0, c2 = 0, c3 = 0, a0 = k0, a1 = k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      const uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
      const uint64_t hi0 = __umul64hi(M0, c0), lo0 = M0 * c0, hi1 = __umul64hi(M1, c2), lo1 = M1 * c2;
      const uint64_t n0 = hi1 ^ c1 ^ a0, n2 = hi0 ^ c3 ^ a1;
      c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
      a0 += 0x9E3779B97F4A7C15ull;
      a1 += 0xBB67AE8584CAA73Bull;
    }
    const uint64_t v[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t i = 4 * b + (uint64_t)j;
      if (i < n) {
        const double u = __dmul_rn((double)(v[j] >> 11), 1.0 / 9007199254740992.0);
        out[i] = (float)__dadd_rn(low, __dmul_rn(range, u));
      }
    }
  }
}
__global__ void __launch_bounds__(256)
k_philox_uniform(uint64_t k0, uint64_t k1, uint64_t n, double low, double range, float *__restrict__ out) {
  philox_uniform_body(k0, k1, n, low, range, out);
}
// the key read from device memory: a captured launch (hipGraph) is re-seeded by rewriting two words
__global__ void __launch_bounds__(256)
k_philox_uniform_devkey(const uint64_t *__restrict__ key, uint64_t n, double low, double range, float *__restrict__ out) {
  philox_uniform_body(key[0], key[1], n, low, range, out);
}
// Edge k of np.linspace(lo, hi, n_bins + 1) in float64, rounding for rounding: fl(fl(k * step) + lo),
// step = fl((hi - lo) / n_bins) (computed on the host), the last edge hi itself.  Separate rounded
// product and sum: an FMA would round once and move the edge.  (__dmul_rn / __dadd_rn are a plain
// * and + in this HIP build, which -ffp-contract=fast fuses; the pragma keeps them apart.)
__device__ __forceinline__ double hist_edge(int k, int n_bins, double lo, double hi, double step) {
#pragma clang fp contract(off)
  const double prod = (double)k * step;
  return k == n_bins ? hi : prod + lo;
}

// numpy.histogram's bin of v over linspace(lo, hi, n_bins + 1) (float64 edges), last bin
// right-inclusive; -1 = dropped.  A float32 estimate, then moved until the float64 edges agree: a
// float32 value just below a float64 edge can round onto the float32 edge.
__device__ __forceinline__ int hist_bin(float v, int n_bins, float lo, float hi, double step) {
  if (!(v >= lo) || !(v <= hi)) return -1;  // numpy drops out-of-range and NaN
  const float scale = (float)n_bins / (hi - lo);
  int bin = (int)((v - lo) * scale);
  bin = bin < 0 ? 0 : bin >= n_bins ? n_bins - 1 : bin;  // right edge inclusive
  const double x = v, dlo = lo, dhi = hi;
  while (bin > 0 && x < hist_edge(bin, n_bins, dlo, dhi, step)) --bin;
  while (bin < n_bins - 1 && x >= hist_edge(bin + 1, n_bins, dlo, dhi, step)) ++bin;
  return bin;
}

__global__ void __launch_bounds__(256)
k_histogram(const float *__restrict__ values, int64_t count, int n_bins, float lo, float hi, double step,
            int *__restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const int bin = hist_bin(values[i], n_bins, lo, hi, step);
    if (bin >= 0) atomicAdd(counts + bin, 1);
  }
}

// <= 4096 bins: every workgroup bins its share in LDS (integer atomics on the LDS crossbar instead
// of contended global ones: 1024 values into 75 bins took 13.8 us + a 5 us memset before).  ONE
// workgroup (SOLO, counts up to 2^16 values): the bins are stored, not added -- no memset launch.
template <bool SOLO>
__global__ void __launch_bounds__(1024)
k_histogram_lds(const float *__restrict__ values, int64_t count, int n_bins, float lo, float hi, double step,
                int *__restrict__ counts) {
  extern __shared__ float4 smem4[];
  int *bins = reinterpret_cast<int *>(smem4);
  for (int k = threadIdx.x; k < n_bins; k += blockDim.x) bins[k] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const int bin = hist_bin(values[i], n_bins, lo, hi, step);
    if (bin >= 0) atomicAdd(bins + bin, 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < n_bins; k += blockDim.x) {
    if (SOLO) counts[k] = bins[k];
    else if (bins[k]) atomicAdd(counts + k, bins[k]);
  }
}


// ---- shot sampling (simulation.py:320-377) ------------------------------------------
// Philox4x32-10 counter RNG: counter = (shot pair, 0, row lo, row hi), key = seed.
struct Philox4 { uint32_t x[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                 uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {  // uniform in (0, 1)
  return ((double)((((uint64_t)hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// Inclusive fp64 prefix sum of one row of probabilities per block: cdf[b][i] = sum_{j<=i} p[b][j]
__global__ void __launch_bounds__(256)
k_cdf(const float *__restrict__ probs, uint64_t D, double *__restrict__ cdf) {
  __shared__ double wsum[4];
  __shared__ double carry_s;
  const float *p = probs + (size_t)blockIdx.x * D;
  double *c = cdf + (size_t)blockIdx.x * D;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0.0;
  __syncthreads();
  for (uint64_t base = 0; base < D; base += 1024) {
    const uint64_t i0 = base + (uint64_t)threadIdx.x * 4;
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (i0 + k < D) ? (double)p[i0 + k] : 0.0;
    v[1] += v[0];
    v[2] += v[1];
    v[3] += v[2];
    double incl = v[3];  // inclusive scan of the per-thread totals across the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    double before = carry_s + (incl - v[3]);
    for (int j = 0; j < w; ++j) before += wsum[j];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < D) c[i0 + k] = before + v[k];
    __syncthreads();
    if (threadIdx.x == 255) carry_s = before + v[3];
    __syncthreads();
  }
}

// First index with cdf[idx] >= r (numpy.searchsorted side="left").
__device__ __forceinline__ uint32_t cdf_search(const double *__restrict__ c, uint64_t D,
                                               double r) {
  uint64_t lo = 0, hi = D - 1;  // answer in [lo, hi]; cdf[D-1] = total >= r
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (c[mid] >= r) hi = mid; else lo = mid + 1;
  }
  return (uint32_t)lo;
}

constexpr int kShotsPerThread = 16;                       // 8 Philox blocks
constexpr int kShotsPerBlock = 256 * kShotsPerThread;     // 4096
constexpr int kLdsHistMax = 4096;                         // bins kept in LDS (16 KiB)

// counts[b][idx] += 1 for `shots` draws idx ~ probs[b]; grid (ceil(shots/4096), rows)
template <bool LDS_HIST>
__global__ void __launch_bounds__(256)
k_sample(const double *__restrict__ cdf, uint64_t D, int shots, uint64_t seed,
         uint64_t row_offset, int *__restrict__ counts) {
  __shared__ int hist[LDS_HIST ? kLdsHistMax : 1];
  const double *c = cdf + (size_t)blockIdx.y * D;
  int *out = counts + (size_t)blockIdx.y * D;
  if (LDS_HIST) {
    for (uint32_t i = threadIdx.x; i < D; i += 256) hist[i] = 0;
    __syncthreads();
  }
  const double total = c[D - 1];
  const uint64_t row = row_offset + blockIdx.y;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int64_t first = (int64_t)blockIdx.x * kShotsPerBlock;
#pragma unroll 1
  for (int j = 0; j < kShotsPerThread / 2; ++j) {
    // shot pair index: consecutive threads take consecutive pairs
    const int64_t pair = first / 2 + (int64_t)j * 256 + threadIdx.x;
    if (2 * pair >= shots) break;
    const Philox4 rnd = philox4x32_10((uint32_t)pair, (uint32_t)((uint64_t)pair >> 32),
                                      (uint32_t)row, (uint32_t)(row >> 32), k0, k1);
    const uint32_t a = cdf_search(c, D, total * u53(rnd.x[0], rnd.x[1]));
    if (LDS_HIST) atomicAdd(&hist[a], 1); else atomicAdd(out + a, 1);
    if (2 * pair + 1 < shots) {
      const uint32_t b = cdf_search(c, D, total * u53(rnd.x[2], rnd.x[3]));
      if (LDS_HIST) atomicAdd(&hist[b], 1); else atomicAdd(out + b, 1);
    }
  }
  if (LDS_HIST) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < D; i += 256)
      if (hist[i]) atomicAdd(out + i, hist[i]);
  }
}

__global__ void __launch_bounds__(256)
k_counts_to_probs(const int *__restrict__ counts, uint64_t total, float inv_shots,
                  float *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
    out[i] = (float)counts[i] * inv_shots;
}

// sum_i p[b][i] * d_k[sub_k(i)]: the diagonal of observable k lifted to the register
// (simulation.py:363-372).  diag_off < 0: Z-parity over the wires (no table).
struct DiagObs {
  int8_t bits[QMLE_MAX_QUBITS];  // bit positions of the observable's wires, MSB first
  int n_wires;
  int diag_off;
};
__global__ void __launch_bounds__(256)
k_probs_diag_expval(const float *__restrict__ probs, uint64_t D, const DiagObs *__restrict__ obs,
                    const float *__restrict__ diag, int n_obs, float *__restrict__ out) {
  __shared__ double red[16];
  const DiagObs ob = obs[blockIdx.y];
  const float *p = probs + (size_t)blockIdx.x * D;
  double acc = 0.0;
  for (uint64_t i = threadIdx.x; i < D; i += 256) {
    uint32_t sub = 0;
    for (int k = 0; k < ob.n_wires; ++k) sub = (sub << 1) | (uint32_t)((i >> ob.bits[k]) & 1);
    const float d = ob.diag_off < 0 ? ((__popc(sub) & 1) ? -1.f : 1.f) : diag[ob.diag_off + sub];
    acc += (double)(p[i] * d);
  }
  const double t = block_sum_d(acc, red);
  if (threadIdx.x == 0) out[(size_t)blockIdx.x * n_obs + blockIdx.y] = (float)t;
}



// <a_i|b_i> for separate arrays a, b: partial[i][block] = (re, im)
__global__ void __launch_bounds__(256)
k_overlap2_partial(const float4 *__restrict__ a_all, const float4 *__restrict__ b_all, int n,
                   float2 *__restrict__ partial) {
  __shared__ float red[16];
  const int pr = blockIdx.y;
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const float4 *a = a_all + (size_t)pr * chunks;
  const float4 *c = b_all + (size_t)pr * chunks;
  float re = 0.f, im = 0.f;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < chunks; k += stride) {
    const float4 x = a[k], y = c[k];
    re += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    im += x.x * y.y - x.y * y.x + x.z * y.w - x.w * y.z;
  }
  const float r = block_sum(re, red);
  const float i = block_sum(im, red);
  if (threadIdx.x == 0) partial[(size_t)pr * gridDim.x + blockIdx.x] = make_float2(r, i);
}

__global__ void __launch_bounds__(256)
k_overlap2_final(const float2 *__restrict__ partial, int n_blocks, int count,
                 float2 *__restrict__ out) {
  __shared__ double red[16];
  const int pr = blockIdx.x;
  double re = 0.0, im = 0.0;
  for (int i = threadIdx.x; i < n_blocks; i += blockDim.x) {
    const float2 v = partial[(size_t)pr * n_blocks + i];
    re += v.x;
    im += v.y;
  }
  re = block_sum_d(re, red);
  im = block_sum_d(im, red);
  if (threadIdx.x == 0) out[pr] = make_float2((float)re, (float)im);
}

// Z-parity expectation: sum_i (-1)^{popcount(i & mask)} |psi_i|^2, up to 8 masks per launch.
struct ParityMasks {
  uint32_t m[8];
  int count;
};

__global__ void __launch_bounds__(256)
k_parity_partial(const float4 *__restrict__ states, int n, ParityMasks pm,
                 float *__restrict__ partial) {
  __shared__ float red[16];
  const int b = blockIdx.y;
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const float4 *st = states + (size_t)b * chunks;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
    const float4 v = st[c];
    const float pe = v.x * v.x + v.y * v.y, po = v.z * v.z + v.w * v.w;
    const uint32_t ie = (uint32_t)(c << 1), io = ie | 1u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      acc[k] += (__popc(ie & pm.m[k]) & 1) ? -pe : pe;
      acc[k] += (__popc(io & pm.m[k]) & 1) ? -po : po;
    }
  }
  float *out = partial + ((size_t)b * gridDim.x + blockIdx.x) * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float r = block_sum(acc[k], red);
    if (threadIdx.x == 0) out[k] = r;
  }
}

__global__ void __launch_bounds__(256)
k_parity_final(const float *__restrict__ partial, int n_blocks, int count, int n_obs_total,
               int obs_off, float *__restrict__ out) {
  __shared__ double red[16];
  const int b = blockIdx.x;
  const float *pp = partial + (size_t)b * n_blocks * 8;
  for (int k = 0; k < count; ++k) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += blockDim.x) acc += (double)pp[(size_t)i * 8 + k];
    const double tot = block_sum_d(acc, red);
    if (threadIdx.x == 0) out[(size_t)b * n_obs_total + obs_off + k] = (float)tot;
  }
}
// vec(rho) measurements: rho[i][j] at flat index i * D + j (ket bits first)
__global__ void __launch_bounds__(256)
k_density_probs(const float2 *__restrict__ rho, int n, float *__restrict__ out) {
  const int b = blockIdx.y;
  const uint64_t D = (uint64_t)1 << n;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D) out[(size_t)b * D + i] = rho[((size_t)b << (2 * n)) + i * (D + 1)].x;
}

__global__ void __launch_bounds__(256)
k_density_expval(const float2 *__restrict__ rho, int n, ObsBits obs, int n_obs,
                 float *__restrict__ out) {
  __shared__ double red[16];
  const int b = blockIdx.x, k = blockIdx.y;
  const uint64_t D = (uint64_t)1 << n;
  const float2 *r = rho + ((size_t)b << (2 * n));
  const int p = obs.bits[k];
  double acc = 0.0;
  for (uint64_t i = threadIdx.x; i < D; i += blockDim.x) {
    const float v = r[i * (D + 1)].x;
    acc += ((i >> p) & 1ull) ? -(double)v : (double)v;
  }
  const double tot = block_sum_d(acc, red);
  if (threadIdx.x == 0) out[(size_t)b * n_obs + k] = (float)tot;
}

}  // namespace

namespace qmle {

int expval_blocks(int n) {
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const uint64_t seg = (uint64_t)kEzThreads * kEzUnroll;
  uint64_t n_seg = (chunks + seg - 1) / seg;
  if (n_seg > 2048) n_seg = 2048;
  return (int)n_seg;
}

int run_expval(const float2 *states, int n, int batch, const int8_t *obs_bits, int n_obs,
               float *d_out, void *ws, size_t ws_bytes, hipStream_t stream) {
  if (n_obs < 1 || n_obs > QMLE_MAX_QUBITS) return QMLE_ERR_INVALID_ARG;
  const int nb = expval_blocks(n);
  const size_t need = (size_t)batch * nb * (QMLE_MAX_QUBITS + 1) * sizeof(float);
  if (ws_bytes < need) return QMLE_ERR_WORKSPACE;
  ObsBits ob;
  for (int k = 0; k < QMLE_MAX_QUBITS; ++k) ob.row_mask[k] = 0u;
  for (int k = 0; k < n_obs; ++k) {
    if (obs_bits[k] < 0 || obs_bits[k] >= n) return QMLE_ERR_WIRE_RANGE;
    ob.bits[k] = obs_bits[k];
  }
  hipLaunchKernelGGL(k_expval_partial, dim3(nb, batch), dim3(kEzThreads), 0, stream,
                     reinterpret_cast<const float4 *>(states), n, (float *)ws);
  hipLaunchKernelGGL(k_expval_final, dim3(batch, n_obs), dim3(256), 0, stream,
                     (const float *)ws, nb, n_obs, ob, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int overlap_blocks(int n) {
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  uint64_t b = (chunks + 256 * 4 - 1) / (256 * 4);
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return (int)b;
}

// Z-parity observables (bit-position masks) of resident states: the stand-alone kernels
int run_parity_pos(const float2 *states, int n, int batch, const uint32_t *pos_masks,
                          int n_obs, float *d_out, void *ws, size_t ws_bytes,
                          hipStream_t stream) {
  const int nb = overlap_blocks(n);
  if (ws_bytes < (size_t)batch * nb * 8 * sizeof(float)) return QMLE_ERR_WORKSPACE;
  for (int o0 = 0; o0 < n_obs; o0 += 8) {
    ParityMasks pm;
    pm.count = n_obs - o0 < 8 ? n_obs - o0 : 8;
    for (int k = 0; k < 8; ++k) pm.m[k] = k < pm.count ? pos_masks[o0 + k] : 0u;
    hipLaunchKernelGGL(k_parity_partial, dim3(nb, batch), dim3(256), 0, stream,
                       (const float4 *)states, n, pm, (float *)ws);
    hipLaunchKernelGGL(k_parity_final, dim3(batch), dim3(nb >= 256 ? 256 : 64), 0, stream,
                       (const float *)ws, nb, pm.count, n_obs, o0, d_out);
  }
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

void launch_expval_final(const float *partial, int n_rows, int batch, int n_obs, const ObsBits &ob,
                         float *d_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_expval_final, dim3(batch, n_obs), dim3(256), 0, stream, partial, n_rows, n_obs, ob, d_out);
}

void launch_probs(const float2 *states, float *d_out, uint64_t total_chunks, hipStream_t stream) {
  hipLaunchKernelGGL(k_probs, dim3(grid_for(total_chunks, 256)), dim3(256), 0, stream,
                     reinterpret_cast<const float4 *>(states), reinterpret_cast<float2 *>(d_out), total_chunks);
}

void launch_density(const float2 *states, float2 *d_out, int n, int batch, hipStream_t stream) {
  const uint64_t D = (uint64_t)1 << n;
  hipLaunchKernelGGL(k_density, dim3(grid_for(D * D, 256, 1u << 20), batch), dim3(256), 0, stream, states, d_out, n);
}

}  // namespace qmle

extern "C" {

size_t qmle_expval_workspace_bytes(int n_qubits, int batch) {
  if (n_qubits < 1 || batch < 1) return 0;
  return (size_t)batch * expval_blocks(n_qubits) * (QMLE_MAX_QUBITS + 1) * sizeof(float) + 256;
}

int qmle_expval_z(const void *d_states, int n_qubits, int batch, const int32_t *obs_wires,
                  int n_obs, float *d_out, void *d_workspace, size_t workspace_bytes,
                  qmle_stream stream) {
  if (!d_states || !d_out || !d_workspace || !obs_wires || n_qubits < 1 ||
      n_qubits > QMLE_MAX_QUBITS || batch < 1 || batch > kMaxGridY)
    return QMLE_ERR_INVALID_ARG;
  if (n_obs < 1 || n_obs > QMLE_MAX_QUBITS) return QMLE_ERR_INVALID_ARG;
  int8_t bits[QMLE_MAX_QUBITS];
  for (int k = 0; k < n_obs; ++k) {
    if (obs_wires[k] < 0 || obs_wires[k] >= n_qubits) return QMLE_ERR_WIRE_RANGE;
    bits[k] = (int8_t)(n_qubits - 1 - obs_wires[k]);
  }
  return run_expval((const float2 *)d_states, n_qubits, batch, bits, n_obs, d_out,
                    d_workspace, workspace_bytes, (hipStream_t)stream);
}

int qmle_probs(const void *d_states, int n_qubits, int batch, float *d_out, qmle_stream stream) {
  if (!d_states || !d_out || n_qubits < 1 || n_qubits > QMLE_MAX_QUBITS || batch < 1)
    return QMLE_ERR_INVALID_ARG;
  launch_probs((const float2 *)d_states, d_out, (uint64_t)batch << (n_qubits - 1), (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_density(const void *d_states, int n_qubits, int batch, void *d_out, qmle_stream stream) {
  if (!d_states || !d_out || n_qubits < 1 || batch < 1 || batch > kMaxGridY) return QMLE_ERR_INVALID_ARG;
  if (n_qubits > 15) return QMLE_ERR_UNSUPPORTED;
  launch_density((const float2 *)d_states, (float2 *)d_out, n_qubits, batch, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_marginal_probs(const void *d_states, int n_qubits, int batch, const int32_t *keep_wires,
                        int n_keep, float *d_out, qmle_stream stream_) {
  if (!d_states || !d_out || !keep_wires || n_qubits < 1 || n_qubits > QMLE_MAX_QUBITS ||
      batch < 1 || batch > kMaxGridY || n_keep < 1 || n_keep > n_qubits || n_keep > 24)
    return QMLE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  // kept wires stay in ascending wire order regardless of `keep` order
  // (jaqsi.py:141-146): output bit k (LSB first) <- the k-th LARGEST wire.
  uint64_t mask = 0;
  for (int k = 0; k < n_keep; ++k) {
    if (keep_wires[k] < 0 || keep_wires[k] >= n_qubits) return QMLE_ERR_WIRE_RANGE;
    if (mask & (1ull << keep_wires[k])) return QMLE_ERR_DUPLICATE_WIRES;
    mask |= 1ull << keep_wires[k];
  }
  KeepBits kb;
  kb.n_keep = n_keep;
  int k = 0;
  for (int w = n_qubits - 1; w >= 0; --w)
    if (mask & (1ull << w)) kb.bits[k++] = (int8_t)(n_qubits - 1 - w);
  HIPCHK(hipMemsetAsync(d_out, 0, ((size_t)batch << n_keep) * sizeof(float), stream));
  const uint64_t D = (uint64_t)1 << n_qubits;
  if (n_keep <= 12) {
    // (<= 512 workgroups per state: >= 2^n / 512 terms are summed in LDS per global atomic)
    hipLaunchKernelGGL(k_marginal_lds, dim3(grid_for(D, 256, 512), batch), dim3(256),
                       sizeof(float) << n_keep, stream, (const float2 *)d_states, d_out, n_qubits, kb);
  } else {
    hipLaunchKernelGGL(k_marginal, dim3(grid_for(D, 256, 4096), batch), dim3(256), 0, stream,
                       (const float2 *)d_states, d_out, n_qubits, kb);
  }
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

size_t qmle_pair_fidelity_workspace_bytes(int n_qubits, int n_pairs) {
  if (n_qubits < 1 || n_pairs < 1) return 0;
  return (size_t)n_pairs * overlap_blocks(n_qubits) * sizeof(float2) + 256;
}

int qmle_pair_fidelity(const void *d_states, int n_qubits, int n_pairs, float *d_out,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream_) {
  if (!d_states || !d_out || !d_workspace || n_qubits < 1 || n_qubits > QMLE_MAX_QUBITS ||
      n_pairs < 1)
    return QMLE_ERR_INVALID_ARG;
  const int nb = overlap_blocks(n_qubits);
  if (workspace_bytes < (size_t)n_pairs * nb * sizeof(float2)) return QMLE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const uint64_t chunks = (uint64_t)1 << (n_qubits - 1);
  if (n_qubits <= 16 && n_pairs >= 64) {  // enough pairs to fill the chip with one workgroup each
    const int threads = chunks >= 256 ? 256 : 64;
    hipLaunchKernelGGL(k_pair_fidelity_small, dim3(n_pairs), dim3(threads), 0, stream,
                       (const float4 *)d_states, n_qubits, n_pairs, d_out);
    HIPCHK(hipGetLastError());
    return QMLE_OK;
  }
  for (int p0 = 0; p0 < n_pairs; p0 += kMaxGridY) {
    const int pc = n_pairs - p0 < kMaxGridY ? n_pairs - p0 : kMaxGridY;
    // pairs (i, i + n_pairs): shift both halves by p0
    hipLaunchKernelGGL(k_overlap_partial, dim3(nb, pc), dim3(256), 0, stream,
                       (const float4 *)d_states + (size_t)p0 * chunks, n_qubits, n_pairs,
                       (float2 *)d_workspace + (size_t)p0 * nb);
  }
  hipLaunchKernelGGL(k_overlap_final, dim3(n_pairs), dim3(nb >= 256 ? 256 : 64), 0, stream,
                     (const float2 *)d_workspace, nb, n_pairs, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_density_probs(const void *d_rho, int n_qubits, int batch, float *d_out,
                       qmle_stream stream) {
  if (!d_rho || !d_out || n_qubits < 1 || 2 * n_qubits > QMLE_MAX_QUBITS || batch < 1 ||
      batch > kMaxGridY)
    return QMLE_ERR_INVALID_ARG;
  const uint64_t D = (uint64_t)1 << n_qubits;
  hipLaunchKernelGGL(k_density_probs, dim3(grid_for(D, 256), batch), dim3(256), 0,
                     (hipStream_t)stream, (const float2 *)d_rho, n_qubits, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_density_expval_z(const void *d_rho, int n_qubits, int batch, const int32_t *obs_wires,
                          int n_obs, float *d_out, qmle_stream stream) {
  if (!d_rho || !d_out || !obs_wires || n_qubits < 1 || 2 * n_qubits > QMLE_MAX_QUBITS ||
      batch < 1 || batch > kMaxGridY || n_obs < 1 || n_obs > QMLE_MAX_QUBITS)
    return QMLE_ERR_INVALID_ARG;
  ObsBits ob;
  for (int k = 0; k < n_obs; ++k) {
    if (obs_wires[k] < 0 || obs_wires[k] >= n_qubits) return QMLE_ERR_WIRE_RANGE;
    ob.bits[k] = (int8_t)(n_qubits - 1 - obs_wires[k]);
  }
  hipLaunchKernelGGL(k_density_expval, dim3(batch, n_obs), dim3(256), 0, (hipStream_t)stream,
                     (const float2 *)d_rho, n_qubits, ob, n_obs, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

size_t qmle_overlap_workspace_bytes(int n_qubits, int count) {
  if (n_qubits < 1 || count < 1) return 0;
  return (size_t)count * overlap_blocks(n_qubits) * sizeof(float2) + 256;
}

int qmle_overlap(const void *d_a, const void *d_b, int n_qubits, int count, void *d_out,
                 void *d_workspace, size_t workspace_bytes, qmle_stream stream_) {
  if (!d_a || !d_b || !d_out || !d_workspace || n_qubits < 1 || n_qubits > QMLE_MAX_QUBITS ||
      count < 1)
    return QMLE_ERR_INVALID_ARG;
  const int nb = overlap_blocks(n_qubits);
  if (workspace_bytes < (size_t)count * nb * sizeof(float2)) return QMLE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const uint64_t chunks = (uint64_t)1 << (n_qubits - 1);
  for (int p0 = 0; p0 < count; p0 += kMaxGridY) {
    const int pc = count - p0 < kMaxGridY ? count - p0 : kMaxGridY;
    hipLaunchKernelGGL(k_overlap2_partial, dim3(nb, pc), dim3(256), 0, stream,
                       (const float4 *)d_a + (size_t)p0 * chunks,
                       (const float4 *)d_b + (size_t)p0 * chunks, n_qubits,
                       (float2 *)d_workspace + (size_t)p0 * nb);
  }
  hipLaunchKernelGGL(k_overlap2_final, dim3(count), dim3(nb >= 256 ? 256 : 64), 0, stream,
                     (const float2 *)d_workspace, nb, count, (float2 *)d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

size_t qmle_expval_parity_workspace_bytes(int n_qubits, int batch) {
  if (n_qubits < 1 || batch < 1) return 0;
  return (size_t)batch * overlap_blocks(n_qubits) * 8 * sizeof(float) + 256;
}

int qmle_expval_parity(const void *d_states, int n_qubits, int batch, const uint32_t *wire_masks,
                       int n_obs, float *d_out, void *d_workspace, size_t workspace_bytes,
                       qmle_stream stream_) {
  if (!d_states || !d_out || !d_workspace || !wire_masks || n_qubits < 1 ||
      n_qubits > QMLE_MAX_QUBITS || batch < 1 || batch > kMaxGridY || n_obs < 1)
    return QMLE_ERR_INVALID_ARG;
  std::vector<uint32_t> pos((size_t)n_obs);
  for (int k = 0; k < n_obs; ++k) {
    // bit w set <=> wire w in the parity (no wire at all is accepted here: the state's norm)
    if (wire_masks[k] != 0 && !valid_wire_mask(wire_masks[k], n_qubits)) return QMLE_ERR_WIRE_RANGE;
    pos[k] = wires_to_pos(wire_masks[k], n_qubits);
  }
  return run_parity_pos((const float2 *)d_states, n_qubits, batch, pos.data(), n_obs, d_out, d_workspace,
                        workspace_bytes, (hipStream_t)stream_);
}

int qmle_philox_uniform_f32_device(const uint64_t key[2], uint64_t n, double low, double high, float *d_out,
                                   qmle_stream stream_) {
  if (!key || (!d_out && n > 0) || n > (1ull << 40)) return QMLE_ERR_INVALID_ARG;
  if (n == 0) return QMLE_OK;
  hipLaunchKernelGGL(k_philox_uniform, dim3(grid_for((n + 3) / 4, 256, 1u << 16)), dim3(256), 0, (hipStream_t)stream_,
                     key[0], key[1], n, low, high - low, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_philox_uniform_f32_device_key(const uint64_t *d_key, uint64_t n, double low, double high, float *d_out,
                                       qmle_stream stream_) {
  if (!d_key || (!d_out && n > 0) || n > (1ull << 40)) return QMLE_ERR_INVALID_ARG;
  if (n == 0) return QMLE_OK;
  hipLaunchKernelGGL(k_philox_uniform_devkey, dim3(grid_for((n + 3) / 4, 256, 1u << 16)), dim3(256), 0,
                     (hipStream_t)stream_, d_key, n, low, high - low, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_histogram(const float *d_values, int64_t count, int n_bins, float lo, float hi,
                   int32_t *d_counts, qmle_stream stream_) {
  if (!d_values || !d_counts || count < 0 || n_bins < 1 || !(hi > lo)) return QMLE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const double step = ((double)hi - (double)lo) / n_bins;  // np.linspace's step (hist_edge)
  if (n_bins <= 4096 && count > 0 && count <= (1 << 16)) {  // one workgroup, one launch
    const int threads = count >= 1024 ? 1024 : count >= 256 ? 256 : 64;
    hipLaunchKernelGGL(k_histogram_lds<true>, dim3(1), dim3(threads), (size_t)n_bins * sizeof(int), stream,
                       d_values, count, n_bins, lo, hi, step, d_counts);
    HIPCHK(hipGetLastError());
    return QMLE_OK;
  }
  HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)n_bins * sizeof(int32_t), stream));
  if (count > 0) {
    if (n_bins <= 4096)
      hipLaunchKernelGGL(k_histogram_lds<false>, dim3(grid_for((uint64_t)count, 1024 * 16, 1024)), dim3(1024),
                         (size_t)n_bins * sizeof(int), stream, d_values, count, n_bins, lo, hi, step, d_counts);
    else
      hipLaunchKernelGGL(k_histogram, dim3(grid_for((uint64_t)count, 256, 1024)), dim3(256), 0,
                         stream, d_values, count, n_bins, lo, hi, step, d_counts);
  }
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

size_t qmle_sample_workspace_bytes(int n_qubits, int batch) {
  if (n_qubits < 1 || n_qubits > QMLE_MAX_QUBITS || batch < 1) return 0;
  return ((size_t)batch << n_qubits) * sizeof(double);
}

int qmle_sample_counts(const float *d_probs, int n_qubits, int batch, int shots, uint64_t seed,
                       uint64_t row_offset, int32_t *d_counts, float *d_est_probs,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream_) {
  if (!d_probs || !d_counts || !d_workspace || n_qubits < 1 || n_qubits > QMLE_MAX_QUBITS ||
      batch < 1 || batch > kMaxGridY || shots < 1)
    return QMLE_ERR_INVALID_ARG;
  if (workspace_bytes < qmle_sample_workspace_bytes(n_qubits, batch))
    return QMLE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const uint64_t D = (uint64_t)1 << n_qubits;
  double *cdf = (double *)d_workspace;
  HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)batch * D * sizeof(int32_t), stream));
  hipLaunchKernelGGL(k_cdf, dim3(batch), dim3(256), 0, stream, d_probs, D, cdf);
  const unsigned gx = (unsigned)(((int64_t)shots + kShotsPerBlock - 1) / kShotsPerBlock);
  if (D <= (uint64_t)kLdsHistMax)
    hipLaunchKernelGGL(k_sample<true>, dim3(gx, batch), dim3(256), 0, stream, cdf, D, shots,
                       seed, row_offset, d_counts);
  else
    hipLaunchKernelGGL(k_sample<false>, dim3(gx, batch), dim3(256), 0, stream, cdf, D, shots,
                       seed, row_offset, d_counts);
  if (d_est_probs)
    hipLaunchKernelGGL(k_counts_to_probs, dim3(grid_for((uint64_t)batch * D, 256, 4096)),
                       dim3(256), 0, stream, d_counts, (uint64_t)batch * D, 1.0f / (float)shots,
                       d_est_probs);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_probs_diag_expval(const float *d_probs, int n_qubits, int batch,
                           const int32_t *obs_wires, const int32_t *obs_n_wires,
                           const int32_t *obs_diag_off, const float *d_diag, int n_obs,
                           float *d_out, void *d_workspace, size_t workspace_bytes,
                           qmle_stream stream_) {
  if (!d_probs || !d_out || !obs_wires || !obs_n_wires || !obs_diag_off || !d_workspace ||
      n_qubits < 1 || n_qubits > QMLE_MAX_QUBITS || batch < 1 || batch > kMaxGridY || n_obs < 1 ||
      n_obs > kMaxGridY)
    return QMLE_ERR_INVALID_ARG;
  if (workspace_bytes < (size_t)n_obs * sizeof(DiagObs)) return QMLE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<DiagObs> host(n_obs);
  int w0 = 0;
  for (int k = 0; k < n_obs; ++k) {
    const int nw = obs_n_wires[k];
    if (nw < 1 || nw > n_qubits) return QMLE_ERR_INVALID_ARG;
    uint32_t seen = 0;
    for (int j = 0; j < nw; ++j) {
      const int w = obs_wires[w0 + j];
      if (w < 0 || w >= n_qubits) return QMLE_ERR_WIRE_RANGE;
      if (seen & (1u << w)) return QMLE_ERR_DUPLICATE_WIRES;
      seen |= 1u << w;
      host[k].bits[j] = (int8_t)(n_qubits - 1 - w);
    }
    host[k].n_wires = nw;
    host[k].diag_off = obs_diag_off[k];
    if (host[k].diag_off >= 0 && !d_diag) return QMLE_ERR_INVALID_ARG;
    w0 += nw;
  }
  HIPCHK(hipMemcpyAsync(d_workspace, host.data(), (size_t)n_obs * sizeof(DiagObs),
                        hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));  // `host` dies with this frame
  hipLaunchKernelGGL(k_probs_diag_expval, dim3(batch, n_obs), dim3(256), 0, stream, d_probs,
                     (uint64_t)1 << n_qubits, (const DiagObs *)d_workspace, d_diag, n_obs, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

size_t qmle_probs_diag_expval_workspace_bytes(int n_obs) {
  return n_obs < 1 ? 0 : (size_t)n_obs * sizeof(DiagObs);
}

}  // extern "C"
