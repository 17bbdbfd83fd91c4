// libqmle_sv, Meyer-Wallach: the read kernels of resident states, the sums behind a producing tile pass, the
// per-wire sweep of small states -- and their host path: one plan of the reads (MwReads), one workspace layout per
// route (MwLayout), one read launcher, three named finishes.  qmle_meyer_wallach_describe writes those decisions
// as JSON without a GPU.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <utility>

#include "qmle_internal.h"
#include "qmle_host.h"
#include "qmle_dev.h"

namespace {

// ---------------------------------------------------------------------------
// Meyer-Wallach (entanglement.py:69-103 with Tr rho_j^2 = a^2 + d^2 + 2 |c|^2): THREE reads of
// the state at n = 28 -- ceil((n - 12) / 8) + 1 in general -- instead of n.
//
// A read streams the state through 2^12-amplitude LDS tiles: the 4 lowest bits (128-byte rows)
// + two runs of 4 bit positions, [lo, lo+4) and [lo2, lo2+4), and reports the cross terms
// c_j = sum_{bit_j = 0} psi_i conj(psi_{i + 2^j}) of its bits.  The FIRST read's tile is 32 KiB
// of contiguous memory (bits 0..11); it also reports the signed populations of those 12 bits and
// the per-row totals from which the populations of EVERY other bit follow (sign of a row = one
// bit of its index), so the later reads carry cross terms only.
//
// Round-3 structure (tools/mw_tune.hip has the stand-alone bench it was tuned with):
//  * a lane's own 8 float4 span local bits {0, 9, 10, 11}: their cross terms (and, first read,
//    the 4-bit population butterfly) come straight out of the load registers, before staging;
//  * then ONE staging round trip and cross-only register gathers: local bits 1..4 and 5..8
//    (first read: 2 x 16 ds_read_b64) resp. 4..7 and, for bit 8 alone, 8 ds_read_b128 over
//    {0, 8, 9, 10} (later reads) -- 192 resp. 128 packed fmas per 16 amplitudes, nothing else;
//  * populations of the thread-mapped local bits 1..8 are the per-thread totals signed by the
//    thread index, applied once in the reduction at the end of a workgroup's walk;
//  * no register prefetch: 91 / 108 VGPRs = 5 / 4 workgroups per CU keep more bytes in flight
//    than a software pipeline at 3 (the round-2 kernel: 128 - 144 VGPRs, 4.1 - 4.85 TB/s);
//  * which positions share a tile matters: at n = 28 the pairs {12-15, 24-27} and {16-19, 20-23}
//    stream at 6.9 TB/s, {12-15, 20-23} at 5.7 and {20-27} at 4.5 (same bytes, same code;
//    profiles/r03_mw_tune.txt) -- mw_plan() pairs the 4-bit chunks outermost with innermost.
// Measured at n = 28 (MI355X): first read 0.34 ms, later reads 0.31 ms each; round 2: 0.52 +
// 2 x 0.44.
// ---------------------------------------------------------------------------
constexpr int kMwT = 12, kMwThreads = 256;
constexpr int kMwRowFirst = 48, kMwRowLater = 16;
constexpr int kMwRowLaterLow = 24;  // a later read that also reports positions 0..3: [16 + 2 p], [17 + 2 p]

struct MwReadArgs {
  const float2 *states;
  float *rows;  // [batch][rows_per_state][kMwRowFirst | kMwRowLater]
  int n, lo, lo2, q;  // tile = bits 0..3 + lo..lo+3 + lo2..lo2+3; 2^q tiles per workgroup
};

// (mw_cross: qmle_dev.h -- the tile kernels' fused Meyer-Wallach epilogue uses it too)
// cross terms of the 4 bits a 16-amplitude register gather spans
template <int B0>
__device__ __forceinline__ void mw_cross16(v2f (&cr)[12], const v2f (&r)[16]) {
  static_for<4>([&](auto t) {
    static_for<8>([&](auto pq) {
      constexpr int lowm = (1 << t) - 1;
      constexpr int c = (((int)pq & ~lowm) << 1) | ((int)pq & lowm);
      mw_cross(cr[B0 + (int)t], r[c], r[c | (1 << t)]);
    });
  });
}

// LOW (later reads behind a fused producing pass, round 5): the read also reports the cross terms of positions
// 0..3 -- bit 0 out of the halves of its own float4s, bits 1..3 out of one more 16-amplitude gather (local bits
// 1..4) -- which the producing pass then need not compute: that pass is bound by its vector arithmetic, a later
// read by HBM with ~55 % of its issue slots free (profiles/r05_mw_sq_resident.txt).
template <bool FIRST, bool NT, bool LOW = false>
__device__ __forceinline__ void mw_read_body(const MwReadArgs &a, float4 *smem4) {
  static_assert(!(FIRST && LOW), "the first read reports every low bit anyway");
  const uint32_t sbo = lds_offset_of(smem4);  // 0: no static LDS (launch side checks lds_base_is_zero)
  const uint32_t tid = threadIdx.x;
  const uint32_t jl = 2u * tid;  // local bits 1..8 from tid, 9..11 from u, bit 0 inside the float4
  const int lo = a.lo, lo2 = a.lo2;
  const uint64_t goff = ((uint64_t)(jl & 15u) | ((uint64_t)((jl >> 4) & 15u) << lo) | ((uint64_t)(jl >> 8) << lo2)) << 3;
  const uint64_t ustep = (uint64_t)1 << (lo2 + 1 + 3);  // local bit 9 = second run's bit 1
  const char *st = reinterpret_cast<const char *>(a.states + ((size_t)blockIdx.y << a.n)) + goff;
  const uint32_t slb = (sw(jl) << 3) + sbo;  // staging address of u = 0; u adds u << 12
  const uint32_t tile0 = blockIdx.x << a.q, n_it = 1u << a.q;
  const uint32_t r0 = lo - 4, r1 = lo2 - lo - 4;  // outer runs [4, lo), [lo+4, lo2), [lo2+4, n)

  // cross terms per reported bit: first read local bit b at cr[b]; later reads new bit k at cr[k]
  // (k < 4: lo + k, else lo2 + k - 4)
  v2f cr[12];
  static_for<12>([&](auto k) { cr[k] = (v2f){0.f, 0.f}; });
  float zin[4] = {0.f, 0.f, 0.f, 0.f}, tot = 0.f, zw[4] = {0.f, 0.f, 0.f, 0.f};
  // (LOW: positions 0..3 at cr[8 .. 11] -- the later reads use cr[0 .. 7] only)

  for (uint32_t it = 0; it < n_it; ++it) {
    const uint32_t t = tile0 + it;
    const uint64_t base = ((uint64_t)(t & ((1u << r0) - 1u)) << 4 | (uint64_t)((t >> r0) & ((1u << r1) - 1u)) << (lo + 4) |
                           (uint64_t)(t >> (r0 + r1)) << (lo2 + 4)) << 3;
    float4 v4[8];
    static_for<8>([&](auto u) { v4[u] = ld4<NT>(reinterpret_cast<const float4 *>(st + base + (uint64_t)u * ustep)); });
    v2f lo_[8], hi_[8];  // the two amplitudes of each float4
    static_for<8>([&](auto u) { lo_[u] = (v2f){v4[u].x, v4[u].y}; hi_[u] = (v2f){v4[u].z, v4[u].w}; });
    // ---- bits held by the lane's own 8 float4: local 0 (halves of a float4) and 9, 10, 11 (u) ----
    if (FIRST) {
      static_for<8>([&](auto u) { mw_cross(cr[0], lo_[u], hi_[u]); });
      float pr[16];
      static_for<8>([&](auto u) {
        const v2f q0 = lo_[u] * lo_[u], q1 = hi_[u] * hi_[u];
        pr[2 * u] = q0.x + q0.y;
        pr[2 * u + 1] = q1.x + q1.y;
      });
      float h0 = 0.f, h1 = 0.f, h2 = 0.f, s1[8], s2[4], s3[2];
      static_for<8>([&](auto i) { s1[i] = pr[2 * i] + pr[2 * i + 1]; h0 += pr[2 * i] - pr[2 * i + 1]; });
      static_for<4>([&](auto i) { s2[i] = s1[2 * i] + s1[2 * i + 1]; h1 += s1[2 * i] - s1[2 * i + 1]; });
      static_for<2>([&](auto i) { s3[i] = s2[2 * i] + s2[2 * i + 1]; h2 += s2[2 * i] - s2[2 * i + 1]; });
      zin[0] += h0; zin[1] += h1; zin[2] += h2; zin[3] += s3[0] - s3[1];
      const float tt = s3[0] + s3[1];
      tot += tt;
      static_for<4>([&](auto j) { zw[j] += __uint_as_float(__float_as_uint(tt) ^ (((it >> j) & 1u) << 31)); });
    }
    if (LOW) static_for<8>([&](auto u) { mw_cross(cr[8], lo_[u], hi_[u]); });
    static_for<3>([&](auto k) {
      constexpr int B = FIRST ? 9 + (int)k : 5 + (int)k;
      static_for<4>([&](auto pq) {
        constexpr int lowm = (1 << k) - 1;
        constexpr int u0 = (((int)pq & ~lowm) << 1) | ((int)pq & lowm);
        mw_cross(cr[B], lo_[u0], lo_[u0 | (1 << k)]);
        mw_cross(cr[B], hi_[u0], hi_[u0 | (1 << k)]);
      });
    });
    if (it) __syncthreads();  // the previous tile's gathers are done
    static_for<8>([&](auto u) { lds_st128(slb + ((uint32_t)u << 12), v4[u]); });
    __syncthreads();
    uint32_t tg = tid;
    asm volatile("" : "+v"(tg));  // keeps the gather addresses out of loop-carried registers
    {  // gather A: 16 amplitudes over local bits gA .. gA+3 (first read 1..4, later reads 4..7)
      constexpr int gA = FIRST ? 1 : 4;
      const uint32_t bs = (sw(ins0(ins0(ins0(ins0(tg, gA), gA + 1), gA + 2), gA + 3)) << 3) + sbo;
      v2f r[16];
      static_for<16>([&](auto c) {
        const u64 x = lds_ld64(bs ^ (sw((uint32_t)c << gA) << 3));
        r[c] = (v2f){__uint_as_float((uint32_t)x), __uint_as_float((uint32_t)(x >> 32))};
      });
      mw_cross16<FIRST ? gA : 0>(cr, r);
    }
    if (FIRST) {  // gather B: local bits 5..8
      constexpr int gB = 5;
      const uint32_t bs = (sw(ins0(ins0(ins0(ins0(tg, gB), gB + 1), gB + 2), gB + 3)) << 3) + sbo;
      v2f r[16];
      static_for<16>([&](auto c) {
        const u64 x = lds_ld64(bs ^ (sw((uint32_t)c << gB) << 3));
        r[c] = (v2f){__uint_as_float((uint32_t)x), __uint_as_float((uint32_t)(x >> 32))};
      });
      mw_cross16<gB>(cr, r);
    } else {
      if (LOW) {  // local bits 1..3 (positions 1..3): the gather over local bits 1..4, its first three bits
        constexpr int gL = 1;
        const uint32_t bs = (sw(ins0(ins0(ins0(ins0(tg, gL), gL + 1), gL + 2), gL + 3)) << 3) + sbo;
        v2f r[16];
        static_for<16>([&](auto c) {
          const u64 x = lds_ld64(bs ^ (sw((uint32_t)c << gL) << 3));
          r[c] = (v2f){__uint_as_float((uint32_t)x), __uint_as_float((uint32_t)(x >> 32))};
        });
        static_for<3>([&](auto t) {
          static_for<8>([&](auto pq) {
            constexpr int lowm = (1 << t) - 1;
            constexpr int c = (((int)pq & ~lowm) << 1) | ((int)pq & lowm);
            mw_cross(cr[9 + (int)t], r[c], r[c | (1 << t)]);
          });
        });
      }
      // local bit 8 alone: 8 float4 over local bits {0, 8, 9, 10}; thread index -> 1..7, 11
      const uint32_t e0 = ((tg & 127u) << 1) | ((tg >> 7) << 11);
      const uint32_t bs = (sw(e0) << 3) + sbo;
      float4 r[8];
      static_for<8>([&](auto c) {
        constexpr uint32_t e = (((uint32_t)c & 1u) << 8) | (((uint32_t)c >> 1) << 9);
        r[c] = lds_ld128(bs ^ (sw(e) << 3));
      });
      static_for<4>([&](auto pq) {
        mw_cross(cr[4], (v2f){r[2 * pq].x, r[2 * pq].y}, (v2f){r[2 * pq + 1].x, r[2 * pq + 1].y});
        mw_cross(cr[4], (v2f){r[2 * pq].z, r[2 * pq].w}, (v2f){r[2 * pq + 1].z, r[2 * pq + 1].w});
      });
    }
  }
  // ---- one reduction and one row per workgroup ----
  // first read: [0..23] cross terms of local bit b at 2b, 2b+1; [24..35] signed populations of
  // local bits 0..11; [36] total; [37..40] total signed by bit j of the tile's index in the walk.
  // later reads: [0..15] cross terms of new bit k at 2k, 2k+1.
  constexpr int NB = (FIRST || LOW) ? 12 : 8, NV = FIRST ? 41 : LOW ? kMwRowLaterLow : kMwRowLater;
  float red_v[NV];
  static_for<NB>([&](auto k) { red_v[2 * k] = cr[k].x; red_v[2 * k + 1] = cr[k].y; });
  if (FIRST) {
    red_v[24] = zin[0];
    static_for<8>([&](auto k) { red_v[25 + k] = ((tid >> k) & 1u) ? -tot : tot; });
    red_v[33] = zin[1]; red_v[34] = zin[2]; red_v[35] = zin[3];
    red_v[36] = tot;
    static_for<4>([&](auto j) { red_v[37 + j] = zw[j]; });
  }
  wave_sums_dpp63(red_v);
  __syncthreads();  // every gather has been read: the tile becomes scratch
  float *red = reinterpret_cast<float *>(smem4);
  const uint32_t lane = tid & (kWave - 1), w = tid / kWave;
  if (lane == kWave - 1) static_for<NV>([&](auto k) { red[w * NV + k] = red_v[k]; });
  __syncthreads();
  if (tid < NV) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kMwThreads / kWave; ++i) s += red[i * NV + tid];
    a.rows[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (FIRST ? kMwRowFirst : LOW ? kMwRowLaterLow : kMwRowLater) + tid] = s;
  }
}
// Two entry points, because the occupancy that suits them differs: the later reads are bound by
// HBM alone and want every workgroup the LDS admits (5 per CU); the first read carries twice the
// arithmetic and runs FASTER at 4 workgroups per CU (0.33 vs 0.42 ms at n = 28, same
// instructions -- five workgroups of it fight over the vector pipe and the LDS between barriers).
template <bool NT>
__global__ void __launch_bounds__(kMwThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) k_mw_read_first(const MwReadArgs a) {
  extern __shared__ float4 smem4[];
  mw_read_body<true, NT>(a, smem4);
}
template <bool NT>
__global__ void __launch_bounds__(kMwThreads) k_mw_read_later(const MwReadArgs a) {
  extern __shared__ float4 smem4[];
  mw_read_body<false, NT>(a, smem4);
}
template <bool NT>
__global__ void __launch_bounds__(kMwThreads) k_mw_read_later_low(const MwReadArgs a) {
  extern __shared__ float4 smem4[];
  mw_read_body<false, NT, true>(a, smem4);
}

// purity of one wire from the per-workgroup rows: one block per (state, bit position)
struct MwPurityArgs {
  const float *first;       // [batch][rows_first][kMwRowFirst]
  const float *later[8];    // [batch][rows_later[r]][kMwRowLater]
  uint32_t rows_first, rows_later[8];
  int q_first, n;
  int8_t src_read[QMLE_MAX_QUBITS], src_col[QMLE_MAX_QUBITS];
};
__global__ void __launch_bounds__(1024)
k_mw_purity(const MwPurityArgs a, float *__restrict__ pur_out /* [batch][n] by bit position */) {
  __shared__ double red[16];
  const int b = blockIdx.x, p = blockIdx.y;
  const float *fr = a.first + (size_t)b * a.rows_first * kMwRowFirst;
  double cr = 0, ci = 0, z = 0, tot = 0;
  for (uint32_t i = threadIdx.x; i < a.rows_first; i += blockDim.x) {
    const float *row = fr + (size_t)i * kMwRowFirst;
    const float t = row[36];
    tot += t;
    if (p < kMwT) { cr += row[2 * p]; ci += row[2 * p + 1]; z += row[24 + p]; }
    else if (p < kMwT + a.q_first) z += row[37 + p - kMwT];
    else z += ((i >> (p - kMwT - a.q_first)) & 1u) ? -(double)t : (double)t;
  }
  if (p >= kMwT) {
    const int r = a.src_read[p] - 1, col = a.src_col[p];
    const float *lr = a.later[r] + (size_t)b * a.rows_later[r] * kMwRowLater;
    for (uint32_t i = threadIdx.x; i < a.rows_later[r]; i += blockDim.x) {
      cr += lr[(size_t)i * kMwRowLater + 2 * col];
      ci += lr[(size_t)i * kMwRowLater + 2 * col + 1];
    }
  }
  cr = block_sum_d(cr, red);
  ci = block_sum_d(ci, red);
  z = block_sum_d(z, red);
  tot = block_sum_d(tot, red);
  if (threadIdx.x == 0) {
    const double pa = 0.5 * (tot + z), pd = 0.5 * (tot - z);
    pur_out[(size_t)b * a.n + p] = (float)(pa * pa + pd * pd + 2.0 * (cr * cr + ci * ci));
  }
}

__global__ void k_mw_tile_q(const float *__restrict__ pur, int n, int batch,
                            float *__restrict__ out, float *__restrict__ purities) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double sum = 0.0;
  for (int p = 0; p < n; ++p) {
    const float v = pur[(size_t)b * n + p];
    sum += v;
    if (purities) purities[(size_t)b * n + (n - 1 - p)] = v;  // index by wire
  }
  out[b] = (float)(2.0 * (1.0 - sum / n));
}
// ---- Meyer-Wallach behind a producing pass (QMLE_MEAS_MEYER_WALLACH) -------------------------
// The circuit's last tile pass left one row of kMwFusedRowA floats per tile (tile_mw_row in
// qmle_tile_dev.h: cross terms and signed populations of the tile's T local bits + the tile's total);
// positions outside that tile take their cross terms from `later` reads of the stored state and their
// populations from the totals signed by the matching bit of the tile index.
constexpr int kMwFusedRowA = 48;  // = kMwFusedRow (qmle_tile_dev.h)
struct MwFusedArgs {
  const float *first;       // [batch][rows_first][kMwFusedRowA]
  const float *later[8];    // [batch][rows_later[r]][kMwRowLater]
  uint32_t rows_first, rows_later[8];
  uint32_t later_stride[8];  // floats per row of later read r (kMwRowLater, or kMwRowLaterLow for the read that reports 0..3)
  int lean;                  // positions 0..3: cross terms from later read 0 (columns 8 + p), not from the producing pass
  int T, n;
  int lg;                   // a row covers 2^lg consecutive tiles (the producing workgroup's walk): outer index
                            // bits < lg come with their own signed totals at [3T + 1 + i]
  int8_t loc[QMLE_MAX_QUBITS];        // position p -> local bit of the producing tile, or -1
  int8_t outer_idx[QMLE_MAX_QUBITS];  // position p -> bit of the tile index, or -1
  int8_t src_read[QMLE_MAX_QUBITS], src_col[QMLE_MAX_QUBITS];  // outer positions: later read (from 0) and its column
};
// gridDim.z = 1: the purity itself; > 1: slice z of the rows -> partial[b][p][z] = (cr, ci, z, tot) in
// fp64, summed by k_mw_purity_final (one block per (state, position) walking 32768 rows -- n = 28, one
// row per tile -- took 0.21 ms: only 28 workgroups were at it)
__global__ void __launch_bounds__(1024)
k_mw_purity_fused(const MwFusedArgs a, float *__restrict__ pur_out /* [batch][n] by bit position */,
                  double *__restrict__ partial) {
  __shared__ double red[16];
  const int b = blockIdx.x, p = blockIdx.y;
  const int T = a.T, j = a.loc[p], oi = a.outer_idx[p], lg = a.lg;
  const float *fr = a.first + (size_t)b * a.rows_first * kMwFusedRowA;
  const uint32_t per = (a.rows_first + gridDim.z - 1) / gridDim.z;
  const uint32_t r_lo = blockIdx.z * per, r_hi = r_lo + per < a.rows_first ? r_lo + per : a.rows_first;
  double cr = 0, ci = 0, z = 0, tot = 0;
  for (uint32_t i = r_lo + threadIdx.x; i < r_hi; i += blockDim.x) {
    const float *row = fr + (size_t)i * kMwFusedRowA;
    const float t = row[3 * T];
    tot += t;
    if (j >= 0) { cr += row[2 * j]; ci += row[2 * j + 1]; z += row[2 * T + j]; }  // (lean: zeros at 2 j for j < 4)
    else if (oi < lg) z += row[3 * T + 1 + oi];  // a bit of the tile's index inside the workgroup's walk
    else z += ((i >> (oi - lg)) & 1u) ? -(double)t : (double)t;
  }
  if (j < 0 || (a.lean && p < 4)) {
    const int r = a.src_read[p], col = a.src_col[p];
    const uint32_t stride = a.later_stride[r];
    const float *lr = a.later[r] + (size_t)b * a.rows_later[r] * stride;
    const uint32_t perl = (a.rows_later[r] + gridDim.z - 1) / gridDim.z;
    const uint32_t l_lo = blockIdx.z * perl, l_hi = l_lo + perl < a.rows_later[r] ? l_lo + perl : a.rows_later[r];
    for (uint32_t i = l_lo + threadIdx.x; i < l_hi; i += blockDim.x) {
      cr += lr[(size_t)i * stride + 2 * col];
      ci += lr[(size_t)i * stride + 2 * col + 1];
    }
  }
  cr = block_sum_d(cr, red);
  ci = block_sum_d(ci, red);
  z = block_sum_d(z, red);
  tot = block_sum_d(tot, red);
  if (threadIdx.x == 0) {
    if (gridDim.z > 1) {
      double *o = partial + (((size_t)b * a.n + p) * gridDim.z + blockIdx.z) * 4;
      o[0] = cr; o[1] = ci; o[2] = z; o[3] = tot;
    } else {
      const double pa = 0.5 * (tot + z), pd = 0.5 * (tot - z);
      pur_out[(size_t)b * a.n + p] = (float)(pa * pa + pd * pd + 2.0 * (cr * cr + ci * ci));
    }
  }
}
__global__ void __launch_bounds__(64)
k_mw_purity_final(const double *__restrict__ partial, int n, int batch, int slices, float *__restrict__ pur_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (state, position)
  if (i >= batch * n) return;
  double cr = 0, ci = 0, z = 0, tot = 0;
  for (int s = 0; s < slices; ++s) {
    const double *o = partial + ((size_t)i * slices + s) * 4;
    cr += o[0]; ci += o[1]; z += o[2]; tot += o[3];
  }
  const double pa = 0.5 * (tot + z), pd = 0.5 * (tot - z);
  pur_out[i] = (float)(pa * pa + pd * pd + 2.0 * (cr * cr + ci * ci));
}
// ---- the same sums in two coalesced steps (round 5; tiled producing passes) ---------------------
// k_mw_purity_fused walks the rows once per POSITION: 28 blocks re-read the 12.6 MB of rows of an n = 28 state
// through the L2 with 4 floats used of every 192-byte row (33 us + 11 us for the slices + 5 us to pack: 6 % of the
// fused call).  k_mw_colsum sums EVERY column of a row matrix in one coalesced sweep (thread = column, block = a
// slice of the rows; the totals signed by the bits of the row index ride along as extra "columns"), for the
// producing pass's rows and each later read's in one launch (blockIdx.z); k_mw_finish_cols turns a state's
// column sums into its purities and Q.
struct MwColsumArgs {
  const float *rows[9];   // [0] the producing pass's rows, [1 + r] later read r
  uint32_t n_rows[9], stride[9];
  int n_cols[9];
  int tot_col, n_signed;  // matrix 0 only: column of the row total, number of row-index bits to sign it by
  int slices;
  double *out[9];         // [batch][slices][n_cols + n_signed]
};
__global__ void __launch_bounds__(256)
k_mw_colsum(const MwColsumArgs a) {
  // thread = (column, one of four row lanes); eight rows in flight per thread -- with one load per iteration the
  // sweep was bound by the latency of 256 dependent round trips (0.13 ms at n = 28), with one row lane by 32
  __shared__ double part[4][64];
  const int m = blockIdx.z, b = blockIdx.y, sl = blockIdx.x, t = threadIdx.x;
  const int c = t & 63, lane = t >> 6;
  const int nc = a.n_cols[m], ns = m == 0 ? a.n_signed : 0;
  const uint32_t per = (a.n_rows[m] + a.slices - 1) / a.slices;
  const uint32_t lo = sl * per, hi = lo + per < a.n_rows[m] ? lo + per : a.n_rows[m];
  const float *base = a.rows[m] + (size_t)b * a.n_rows[m] * a.stride[m];
  double sum = 0.0;
  if (c < nc + ns) {
    const bool signedc = c >= nc;
    const int k = signedc ? c - nc : 0;
    const uint32_t cidx = signedc ? (uint32_t)a.tot_col : (uint32_t)c, stride = a.stride[m];
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t i = lo + (uint32_t)lane;
    for (; i + 28 < hi; i += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = base[(size_t)(i + 4 * u) * stride + cidx];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += (signedc && (((i + 4 * u) >> k) & 1u)) ? -(double)v[u] : (double)v[u];
    }
    for (; i < hi; i += 4) {
      const double v = (double)base[(size_t)i * stride + cidx];
      acc[0] += (signedc && ((i >> k) & 1u)) ? -v : v;
    }
    sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
  part[lane][c] = sum;
  __syncthreads();
  if (lane == 0 && c < nc + ns)
    a.out[m][((size_t)b * a.slices + sl) * (nc + ns) + c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}
// one block per state: the slices of EVERY matrix are summed at once by all 1024 threads (thread = one of the <= 128
// columns of all matrices side by side x one of 8 slice lanes: coalesced, four loads in flight), then thread p = bit
// position turns the sums into its purity and a wave sum into Q.  (A first form with one thread per position walking
// the slices itself was latency-bound: 1800 dependent loads, 0.43 ms.)
constexpr int kMwColsMax = 128;
__global__ void __launch_bounds__(1024)
k_mw_finish_cols(const MwFusedArgs a, const MwColsumArgs c, int n_mats, float *__restrict__ out /* [batch][n + 1] */) {
  __shared__ double lane_sum[8][kMwColsMax];
  __shared__ double fin[kMwColsMax];
  __shared__ int off[10];
  const int b = blockIdx.x, t = threadIdx.x, col = t & (kMwColsMax - 1), q = t / kMwColsMax;
  if (t == 0) {
    int o = 0;
    for (int m = 0; m < n_mats; ++m) { off[m] = o; o += c.n_cols[m] + (m == 0 ? c.n_signed : 0); }
    off[n_mats] = o;
  }
  __syncthreads();
  {
    int m = 0;
    while (m + 1 < n_mats && col >= off[m + 1]) ++m;
    double acc = 0.0;
    if (col < off[n_mats]) {
      const int w = off[m + 1] - off[m];
      const double *o = c.out[m] + (size_t)b * c.slices * w + (col - off[m]);
      double a4[4] = {0, 0, 0, 0};
      int sl = q;
      for (; sl + 24 < c.slices; sl += 32) {  // four independent loads per round
#pragma unroll
        for (int u = 0; u < 4; ++u) a4[u] += o[(size_t)(sl + 8 * u) * w];
      }
      for (; sl < c.slices; sl += 8) a4[0] += o[(size_t)sl * w];
      acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    }
    lane_sum[q][col] = acc;
  }
  __syncthreads();
  if (q == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += lane_sum[k][col];
    fin[col] = s;
  }
  __syncthreads();
  const int p = t, T = a.T, n = a.n, lg = a.lg;
  if (t >= kWave) return;
  double pur = 0.0;
  if (p < n) {
    const int j = a.loc[p], oi = a.outer_idx[p];
    const double tot = fin[3 * T];
    double cr = 0.0, ci = 0.0, z;
    if (j >= 0) {
      z = fin[2 * T + j];
      if (!(a.lean && p < 4)) { cr = fin[2 * j]; ci = fin[2 * j + 1]; }
    } else if (oi < lg) z = fin[3 * T + 1 + oi];
    else z = fin[c.n_cols[0] + (oi - lg)];
    if (j < 0 || (a.lean && p < 4)) {
      const int r = a.src_read[p], cc = a.src_col[p];
      cr += fin[off[1 + r] + 2 * cc];
      ci += fin[off[1 + r] + 2 * cc + 1];
    }
    const double pa = 0.5 * (tot + z), pd = 0.5 * (tot - z);
    pur = (double)(float)(pa * pa + pd * pd + 2.0 * (cr * cr + ci * ci));  // (rounded like k_mw_purity_fused's store)
    out[(size_t)b * (n + 1) + 1 + (n - 1 - p)] = (float)pur;  // index by wire
  }
  const double sum = wave_sum_d(pur);
  if (p == 0) out[(size_t)b * (n + 1)] = (float)(2.0 * (1.0 - sum / n));
}

// Whole-state plans: ONE row per state and every position local to the producing tile -- purities and Q of a
// state from its row in one work item (the same fp64 arithmetic as k_mw_purity_fused + k_mw_pack, whose
// 24 576 one-row workgroups took 16 + 5 us of the 12-qubit sampling loop's 185)
__global__ void __launch_bounds__(64)
k_mw_whole_state_finish(const MwFusedArgs a, int batch, float *__restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const float *row = a.first + (size_t)b * kMwFusedRowA;
  const int T = a.T, n = a.n;
  const double tot = (double)row[3 * T];
  float *o = out + (size_t)b * (n + 1);
  double sum = 0.0;
  for (int p = 0; p < n; ++p) {
    const int j = a.loc[p];
    const double cr = (double)row[2 * j], ci = (double)row[2 * j + 1], z = (double)row[2 * T + j];
    const double pa = 0.5 * (tot + z), pd = 0.5 * (tot - z);
    const float v = (float)(pa * pa + pd * pd + 2.0 * (cr * cr + ci * ci));
    sum += v;
    o[1 + (n - 1 - p)] = v;  // index by wire
  }
  o[0] = (float)(2.0 * (1.0 - sum / n));
}
// (Q [batch], purities by wire [batch][n]) -> out[b] = (Q, purities by wire)
__global__ void k_mw_pack_wires(const float *__restrict__ q, const float *__restrict__ pur, int n, int batch,
                                float *__restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  float *o = out + (size_t)b * (n + 1);
  o[0] = q[b];
  for (int w = 0; w < n; ++w) o[1 + w] = pur[(size_t)b * n + w];
}
// out[b] = (Q, purity of wire 0, ..., purity of wire n-1)
__global__ void k_mw_pack(const float *__restrict__ pur, int n, int batch, float *__restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double sum = 0.0;
  float *o = out + (size_t)b * (n + 1);
  for (int p = 0; p < n; ++p) {
    const float v = pur[(size_t)b * n + p];
    sum += v;
    o[1 + (n - 1 - p)] = v;  // index by wire
  }
  o[0] = (float)(2.0 * (1.0 - sum / n));
}

// ---- below the tile size (n < 12) ----
// Meyer-Wallach cross terms c_j = sum_{bit_j = 0} psi_i conj(psi_{i + 2^j}) plus the
// populations a_j, d_j; one launch per bit (v1: n reads of the state).
// partial[b][bit][block] = (re c, im c, a, d)
__global__ void __launch_bounds__(256)
k_cross_partial(const float4 *__restrict__ states, int n, int p, float4 *__restrict__ partial,
                int n_blocks) {
  __shared__ float red[16];
  const int b = blockIdx.y;
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const float4 *st = states + (size_t)b * chunks;
  float cr = 0.f, ci = 0.f, pa = 0.f, pd = 0.f;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  if (p == 0) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < chunks; k += stride) {
      const float4 v = st[k];
      cr += v.x * v.z + v.y * v.w;
      ci += v.y * v.z - v.x * v.w;
      pa += v.x * v.x + v.y * v.y;
      pd += v.z * v.z + v.w * v.w;
    }
  } else {
    const uint64_t items = chunks >> 1;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < items; k += stride) {
      const uint64_t c0 = ins0_64(k, p - 1), c1 = c0 | (1ull << (p - 1));
      const float4 x = st[c0], y = st[c1];
      cr += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
      ci += x.y * y.x - x.x * y.y + x.w * y.z - x.z * y.w;
      pa += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
      pd += y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w;
    }
  }
  const float r0 = block_sum(cr, red), r1 = block_sum(ci, red), r2 = block_sum(pa, red),
              r3 = block_sum(pd, red);
  if (threadIdx.x == 0)
    partial[((size_t)b * n + p) * n_blocks + blockIdx.x] = make_float4(r0, r1, r2, r3);
}

__global__ void __launch_bounds__(256)
k_mw_final(const float4 *__restrict__ partial, int n, int n_blocks, int batch,
           float *__restrict__ out, float *__restrict__ purities) {
  __shared__ double red[16];
  const int b = blockIdx.x;
  double sum = 0.0;
  for (int p = 0; p < n; ++p) {
    double cr = 0, ci = 0, a = 0, d = 0;
    for (int i = threadIdx.x; i < n_blocks; i += blockDim.x) {
      const float4 v = partial[((size_t)b * n + p) * n_blocks + i];
      cr += v.x; ci += v.y; a += v.z; d += v.w;
    }
    cr = block_sum_d(cr, red);
    ci = block_sum_d(ci, red);
    a = block_sum_d(a, red);
    d = block_sum_d(d, red);
    if (threadIdx.x == 0) {
      const double pur = a * a + d * d + 2.0 * (cr * cr + ci * ci);
      if (purities) purities[(size_t)b * n + (n - 1 - p)] = (float)pur;  // index by wire
      sum += pur;
    }
  }
  if (threadIdx.x == 0) out[b] = (float)(2.0 * (1.0 - sum / n));
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  Two routes share everything below:
//   stand-alone  qmle_meyer_wallach (and run_mw_resident, which packs its result like the fused route): the first
//                read reports positions 0..11, later reads the rest
//   fused        run_mw_fused: the plan's last tile pass reported its tile's positions, later reads the rest
// ---------------------------------------------------------------------------------------------------------

// ---- the plan of the reads ----
// A later read reports the cross terms of two runs of four positions [lo, lo + 4), [lo2, lo2 + 4) with 4 <= lo,
// lo + 4 <= lo2, lo2 + 4 <= n.  Later reads are numbered from 0; the first read (stand-alone) or the producing
// pass (fused) is kMwFromFirst.
constexpr int kMwMaxLater = 8;
constexpr int kMwFromFirst = -1;  // MwReads::src_read: the first read / the producing pass reports the position
constexpr int kMwNoSource = -2;   // nobody does (while the plan is built; a plan that keeps one is not ok)
struct MwReads {
  int n_later = 0;
  int lo[kMwMaxLater] = {}, lo2[kMwMaxLater] = {}, q[kMwMaxLater] = {};  // 2^q tiles per workgroup
  uint32_t rows[kMwMaxLater] = {};                                       // per state
  int stride[kMwMaxLater] = {};  // floats per row: kMwRowLater, or kMwRowLaterLow for the read that also reports 0..3
  int q_first = 0;               // the stand-alone route's first read
  uint32_t rows_first = 0;
  int src_read[QMLE_MAX_QUBITS], src_col[QMLE_MAX_QUBITS];  // position p: who reports its cross terms, in which column
  bool ok = true;
  MwReads() {  // no later read: everything comes from the first read / the producing pass
    for (int p = 0; p < QMLE_MAX_QUBITS; ++p) { src_read[p] = kMwFromFirst; src_col[p] = -1; }
  }
};
// which two runs share a read
enum MwPairing { kMwPairEnds, kMwPairNeighbours };
struct MwPair { int a, b; };  // b < 0: an odd run

// tiles per workgroup: the first read keeps ~40 sums per work item, a long walk amortises its
// reduction (2^4); the later reads stream best at 2^2 (tools/mw_tune.hip); never fewer than
// ~2048 workgroups per launch
int mw_pick_q(int want, int batch, uint32_t tiles) {
  int q = 0;
  while (q < want && (((uint64_t)batch * tiles) >> (q + 1)) >= 2048) ++q;
  return q;
}

// Step 1, runs: the positions >= 4 that `have` lacks (bit p set <=> position p is reported already) are cut into
// 4-bit runs from the bottom, the last one aligned to the top [n - 4, n).  A resident state has positions 0..11
// from its first read: [12,16), [16,20), ...  A run may overlap its neighbour (n not a multiple of 4).
// -> the number of runs, -1: more than a plan holds.
int mw_choose_runs(int n, uint32_t have, int (&runs)[kMwMaxLater]) {
  int nc = 0, covered_to = 0;
  for (int p = 4; p < n; ++p) {
    if (((have >> p) & 1u) || p < covered_to) continue;
    if (nc == kMwMaxLater) return -1;
    runs[nc] = p + 4 <= n ? p : n - 4;
    covered_to = runs[nc++] + 4;
  }
  return nc;
}

// Step 2, pairs: a later read takes two runs.
// kMwPairEnds (the stand-alone reads): paired outermost with innermost -- at n = 28: {12-15, 24-27} and
// {16-19, 20-23}, the pairs that stream fastest (see the note above k_mw_read).
// kMwPairNeighbours (behind a producing pass):
// (four runs: which two share a read decides how the read streams.  Neighbours share one: measured at n = 28 behind
// the K2-style last tile {0..6, 23..27}, 0.792 ms after the circuit against 0.801 for outermost with innermost (the
// stand-alone reads' rule) or alternate runs, profiles/r05_mw_pairing_nt.txt)
int mw_pair_runs(int (&runs)[kMwMaxLater], int nc, MwPairing rule, MwPair (&pairs)[kMwMaxLater]) {
  if (rule == kMwPairNeighbours && nc == 4) std::swap(runs[1], runs[3]);  // (0,1) (2,3): the loop pairs (c0,c3') = (0,1), (c1',c2) = (3,2)
  int np = 0;
  for (int i = 0, j = nc - 1; i <= j; ++i, --j) pairs[np++] = MwPair{runs[i], i < j ? runs[j] : -1};
  return np;
}

// Step 3, a whole read from a pair.  An odd run is paired with a lower, already reported one (any other run completes
// the read); overlapping runs (the last one is clamped to n - 4) shift the lower one down.  false: no read of the
// kernel's shape holds the pair.
bool mw_complete_pair(int n, MwPair &pr) {
  int a = pr.a, b = pr.b;
  if (b < 0) {  // odd one out
    b = a;
    a = b >= 16 ? 8 : b >= 8 ? b - 4 : -1;
    if (a < 0) { a = b; b = a + 4; if (b + 4 > n) return false; }
  }
  if (a > b) std::swap(a, b);
  if (b < a + 4) a = b - 4;
  if (a < 4) return false;
  pr = MwPair{a, b};
  return true;
}

// The builder: runs, pairs, whole reads, then step 4, sources -- every position takes its sums from the first read
// that reports it.  `have` holds positions 0..3 (every read's tile does).
MwReads mw_build_reads(int n, int batch, uint32_t have, MwPairing rule) {
  MwReads rd;
  for (int p = 0; p < QMLE_MAX_QUBITS; ++p) {
    rd.src_read[p] = p < n && !((have >> p) & 1u) ? kMwNoSource : kMwFromFirst;
    rd.src_col[p] = -1;
  }
  rd.ok = false;
  if ((have & 0xFu) != 0xFu || n < kMwT) return rd;
  int runs[kMwMaxLater];
  MwPair pairs[kMwMaxLater];
  const int nc = mw_choose_runs(n, have, runs);
  if (nc < 0) return rd;
  const int np = mw_pair_runs(runs, nc, rule, pairs);
  const uint32_t tiles = 1u << (n - kMwT);
  for (int i = 0; i < np; ++i) {
    if (!mw_complete_pair(n, pairs[i])) return rd;
    const int r = rd.n_later++;
    rd.lo[r] = pairs[i].a;
    rd.lo2[r] = pairs[i].b;
    rd.q[r] = mw_pick_q(2, batch, tiles);
    rd.rows[r] = tiles >> rd.q[r];
    rd.stride[r] = kMwRowLater;
    for (int k = 0; k < 8; ++k) {
      const int p = k < 4 ? rd.lo[r] + k : rd.lo2[r] + k - 4;
      if (p < n && rd.src_read[p] == kMwNoSource) { rd.src_read[p] = r; rd.src_col[p] = k; }
    }
  }
  rd.ok = true;
  for (int p = 0; p < n; ++p)
    if (rd.src_read[p] == kMwNoSource) rd.ok = false;
  return rd;
}

// resident state (n >= kMwT): the first read reports positions 0..11, position p in column p
MwReads mw_reads_standalone(int n, int batch) {
  MwReads rd = mw_build_reads(n, batch, (1u << kMwT) - 1u, kMwPairEnds);
  for (int p = 0; p < kMwT; ++p) rd.src_col[p] = p;
  const uint32_t tiles = 1u << (n - kMwT);
  rd.q_first = mw_pick_q(4, batch, tiles);
  rd.rows_first = tiles >> rd.q_first;
  return rd;
}

uint32_t stage_tile_mask(const Stage &st) {
  uint32_t m = 0;
  for (int j = 0; j < st.T; ++j) m |= 1u << st.tile_bits[j];
  return m;
}

// behind the producing pass `last`: later reads for the positions outside its tile (none: the tile is the state).
// lean: the first later read also reports positions 0..3, in columns 8..11 of a longer row.
MwReads mw_reads_fused(int n, int batch, const Stage &last, bool lean) {
  if (last.T == n) return MwReads{};
  MwReads rd = mw_build_reads(n, batch, stage_tile_mask(last), kMwPairNeighbours);
  if (lean && rd.ok && rd.n_later >= 1) {
    rd.stride[0] = kMwRowLaterLow;
    for (int p = 0; p < 4; ++p) { rd.src_read[p] = 0; rd.src_col[p] = 8 + p; }
  }
  return rd;
}

uint32_t mw_most_rows(uint32_t rows_first, const MwReads &rd) {
  uint32_t most = rows_first;
  for (int r = 0; r < rd.n_later; ++r) most = std::max(most, rd.rows[r]);
  return most;
}

// ---- the finishes of a fused call (MwFinish, kMwFinishNames: qmle_internal.h) ----
// whole-state: one row per state, every position local to the producing tile (k_mw_whole_state_finish);
// columns: k_mw_colsum + k_mw_finish_cols, while the row matrices are narrow enough for their thread = column maps;
// per-position: k_mw_purity_fused over slices of the rows (+ k_mw_purity_final) + k_mw_pack -- the general one, valid
// for every tiled state; per_position asks for it wherever it is (QMLE_MW_FINISH_PER_POSITION, tests).
// lg: a row of the producing pass covers 2^lg tiles.
constexpr int kMwWholeStateThreads = 64, kMwColsumThreads = 256;  // the block sizes those kernels are written for
MwFinish mw_fused_finish(int n, int T, int lg, const MwReads &rd, bool per_position) {
  const uint32_t rows_first = (1u << (n - T)) >> lg;
  if (T == n && rows_first == 1) return kMwFinishWholeState;
  int colsum_w0 = kMwFusedRowA + (n - T - lg > 0 ? n - T - lg : 0), colsum_w = colsum_w0;
  for (int r = 0; r < rd.n_later; ++r) colsum_w += rd.stride[r];
  if (T < n && !per_position && 3 * T + 5 <= kMwFusedRowA && colsum_w0 <= 64 && colsum_w <= kMwColsMax)
    return kMwFinishColumns;
  return kMwFinishPerPosition;
}

int mw_colsum_slices(uint32_t most_rows) {  // >= 64 rows per block, <= 256 blocks per state and matrix
  int slices = 1;
  while (slices < 256 && (most_rows >> 6) > (uint32_t)slices) slices *= 2;
  return slices;
}
// enough workgroups for the row sums: slices of >= 256 rows, <= 64 per (state, position)
int mw_purity_slices(uint32_t most_rows, int batch, int n) {
  int slices = 1;
  while (slices < 64 && (most_rows >> 8) > (uint32_t)slices && (uint64_t)batch * n * slices < 4096) slices *= 2;
  return slices;
}

// ---- the workspace, one layout per route ----
// What the size queries have always reported beyond the regions; nothing is placed there.
constexpr size_t kMwStandalonePad = 512;  // qmle_meyer_wallach_workspace_bytes, n >= kMwT
constexpr size_t kMwSweepPad = 256;       // ... n < kMwT
constexpr size_t kMwPackedPad = 256;      // mw_resident_ws_bytes, beside one float per state
constexpr size_t kMwFusedPad = 1024;      // mw_fused_ws_bytes
constexpr size_t kMwColsumPad = 64;       // ... with column sums
// the per-position finish's slice partials: < 8192 (state, position, slice) sums of four doubles
constexpr size_t kMwSliceReserve = (size_t)8192 * 4 * sizeof(double);

struct MwRegion { size_t off = 0, bytes = 0; };
struct MwLayout {
  MwRegion first, later[kMwMaxLater];  // rows of the first read / the producing pass, of later read r
  MwRegion pur, partial;               // purities by position; slice partials (fused) / the per-wire sweep's rows
  MwRegion colsum[1 + kMwMaxLater];    // column sums of the producing pass's rows and of each later read's
  MwRegion packed_q, packed_pur;       // run_mw_resident: Q and the purities by wire, before they are packed
  MwFinish finish = kMwFinishPerPosition;
  int slices = 1;    // of the finish
  int finish_threads = 0;  // of the finish's first launch (fused route; 0: no such finish)
  size_t end = 0;    // where the last region ends: what a run checks its workspace against
  size_t total = 0;  // what the size query reports, >= end
};
void mw_place(MwLayout &L, MwRegion &r, size_t bytes, size_t align = sizeof(float)) {
  r.off = align_up(L.end, align);
  r.bytes = bytes;
  L.end = r.off + bytes;
}

// The engine sizes a chunk's workspace as batch x align_up(total(n, 1), 256) and runs chunks of any batch b in it, so
// both layouts keep total(b) <= b * align_up(total(1), 256): rows per state only shrink as the batch grows (mw_pick_q),
// slices with them, and every constant term is counted once per state at batch 1
// (tests/test_mw_layout_cpu.py checks it).
MwLayout mw_layout_standalone(int n, int batch, const MwReads &rd, bool packed) {
  MwLayout L;
  const size_t B = (size_t)batch;
  if (n >= kMwT) {
    mw_place(L, L.first, B * rd.rows_first * kMwRowFirst * sizeof(float));
    for (int r = 0; r < rd.n_later; ++r) mw_place(L, L.later[r], B * rd.rows[r] * rd.stride[r] * sizeof(float));
    L.total = L.end + B * QMLE_MAX_QUBITS * sizeof(float) + kMwStandalonePad;
    mw_place(L, L.pur, B * n * sizeof(float));
  } else {  // one sweep per wire: partial[b][wire][block] = (re c, im c, a, d)
    mw_place(L, L.partial, B * n * overlap_blocks(n) * sizeof(float4));
    L.total = L.end + kMwSweepPad;
  }
  if (packed) {
    L.end = L.total;
    mw_place(L, L.packed_q, B * sizeof(float), 256);
    mw_place(L, L.packed_pur, B * n * sizeof(float));
    L.total = L.packed_q.off + B * (n + 2) * sizeof(float) + kMwPackedPad;
  }
  return L;
}

// The producing pass wrote `first` (one row per 2^row_shift tiles, room for one per tile).  The regions follow the
// call's own reads and finish; the total is sized for every call on these (n, batch, tile): either row length of the
// first later read, any row_shift and either of the two finishes of a tiled state -- QMLE_MW_NO_LEAN is read per
// call, after the workspace was sized, and so is QMLE_MW_FINISH_PER_POSITION (per_position).
MwLayout mw_layout_fused(int n, int batch, const MwReads &rd, int T, int row_shift, bool per_position) {
  MwLayout L;
  const size_t B = (size_t)batch;
  const uint32_t tiles = 1u << (n - T);
  mw_place(L, L.first, B * tiles * kMwFusedRowA * sizeof(float));
  for (int r = 0; r < rd.n_later; ++r) mw_place(L, L.later[r], B * rd.rows[r] * rd.stride[r] * sizeof(float));
  const size_t rows_end = L.end;
  const uint32_t most = mw_most_rows(tiles >> row_shift, rd);
  L.finish = mw_fused_finish(n, T, row_shift, rd, per_position);
  if (L.finish == kMwFinishColumns) {
    L.slices = mw_colsum_slices(most);
    L.finish_threads = kMwColsumThreads;
    const int n_signed = n - T - row_shift > 0 ? n - T - row_shift : 0;
    mw_place(L, L.colsum[0], B * L.slices * (kMwFusedRowA + n_signed) * sizeof(double), sizeof(double));
    for (int r = 0; r < rd.n_later; ++r)
      mw_place(L, L.colsum[1 + r], B * L.slices * rd.stride[r] * sizeof(double), sizeof(double));
  } else if (L.finish == kMwFinishPerPosition) {
    L.slices = mw_purity_slices(most, batch, n);
    L.finish_threads = most / L.slices >= 1024 ? 1024 : most / L.slices >= 256 ? 256 : 64;
    mw_place(L, L.pur, B * QMLE_MAX_QUBITS * sizeof(float));
    mw_place(L, L.partial, L.slices > 1 ? B * n * L.slices * 4 * sizeof(double) : 0, sizeof(double));
  } else {
    L.finish_threads = kMwWholeStateThreads;
  }
  size_t low_rows = 0;  // (either row length fits)
  for (int r = 0; r < rd.n_later; ++r) low_rows += B * rd.rows[r] * (kMwRowLaterLow - rd.stride[r]) * sizeof(float);
  size_t colsum = 0;  // k_mw_colsum's slices (tiled producing passes only)
  if (T < n)
    colsum = B * mw_colsum_slices(mw_most_rows(tiles, rd)) *
                 (kMwFusedRowA + QMLE_MAX_QUBITS + (size_t)rd.n_later * kMwRowLaterLow) * sizeof(double) + kMwColsumPad;
  L.total = rows_end + low_rows + B * QMLE_MAX_QUBITS * sizeof(float) + kMwSliceReserve + kMwFusedPad + colsum;
  return L;
}

// ---- launches ----
enum MwReadKind { kMwReadFirst, kMwReadLater, kMwReadLaterLow };
const char *const kMwReadKindNames[] = {"first", "later", "later_low"};

// One read of the states.  The kernels address their tile by XOR: no static LDS (checked once per device).
int mw_launch_read(MwReadKind kind, bool nt, dim3 grid, const MwReadArgs &a, hipStream_t stream) {
  using Kernel = void (*)(const MwReadArgs);
  static const Kernel kernels[3][2] = {{k_mw_read_first<false>, k_mw_read_first<true>},
                                       {k_mw_read_later<false>, k_mw_read_later<true>},
                                       {k_mw_read_later_low<false>, k_mw_read_later_low<true>}};
  if (FirstUse once{0}; once.first) {
    for (const auto &k : kernels) {
      QMLE_LDS_BASE_CHECK(k[0]);
      QMLE_LDS_BASE_CHECK(k[1]);
    }
    once.done();
  }
  hipLaunchKernelGGL(kernels[kind][nt ? 1 : 0], grid, dim3(kMwThreads), (size_t)8 << kMwT, stream, a);
  return QMLE_OK;
}

// every later read of the plan, rows into L.later[r]
int mw_issue_later_reads(const float2 *states, int n, int batch, const MwReads &rd, const MwLayout &L, char *ws,
                         hipStream_t stream) {
  const uint32_t tiles = 1u << (n - kMwT);
  const bool nt = launch_streams_past_caches((uint64_t)batch, n);
  for (int r = 0; r < rd.n_later; ++r) {
    const MwReadArgs a{states, (float *)(ws + L.later[r].off), n, rd.lo[r], rd.lo2[r], rd.q[r]};
    const int rc = mw_launch_read(rd.stride[r] == kMwRowLaterLow ? kMwReadLaterLow : kMwReadLater, nt,
                                  dim3(tiles >> rd.q[r], batch), a, stream);
    if (rc != QMLE_OK) return rc;
  }
  return QMLE_OK;
}

// LDS-staged tiles: 1 + ceil((n - 12) / 8) reads of the state, then one block per (state, position)
int mw_run_tiled(const float2 *states, int n, int batch, float *d_out, float *d_purities, char *ws, const MwReads &rd,
                 const MwLayout &L, hipStream_t stream) {
  MwPurityArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  pa.first = (const float *)(ws + L.first.off);
  pa.rows_first = rd.rows_first;
  pa.q_first = rd.q_first;
  pa.n = n;
  for (int r = 0; r < rd.n_later; ++r) {
    pa.later[r] = (const float *)(ws + L.later[r].off);
    pa.rows_later[r] = rd.rows[r];
  }
  // (k_mw_purity counts the first read as 0 and later read r as r + 1)
  for (int p = 0; p < n; ++p) {
    pa.src_read[p] = (int8_t)(rd.src_read[p] == kMwFromFirst ? 0 : rd.src_read[p] + 1);
    pa.src_col[p] = (int8_t)rd.src_col[p];
  }
  // The reads are independent of each other.  The first read is the arithmetic-heavy one (192
  // packed fmas + the population butterfly per 16 amplitudes) and is the one that suffers when
  // it starts on a chip that has just idled through the tiny reduction kernels of a previous
  // call (0.33 ms warm, 0.42 - 0.47 ms cold at n = 28); the later reads are bound by HBM
  // alone.  So it runs LAST.
  int rc = mw_issue_later_reads(states, n, batch, rd, L, ws, stream);
  if (rc != QMLE_OK) return rc;
  const MwReadArgs a_first{states, (float *)(ws + L.first.off), n, 4, 8, rd.q_first};
  rc = mw_launch_read(kMwReadFirst, launch_streams_past_caches((uint64_t)batch, n),
                      dim3((1u << (n - kMwT)) >> rd.q_first, batch), a_first, stream);
  if (rc != QMLE_OK) return rc;
  float *d_pur = (float *)(ws + L.pur.off);
  hipLaunchKernelGGL(k_mw_purity, dim3(batch, n), dim3(rd.rows_first >= 1024 ? 1024 : rd.rows_first >= 256 ? 256 : 64),
                     0, stream, pa, d_pur);
  hipLaunchKernelGGL(k_mw_tile_q, dim3((batch + 63) / 64), dim3(64), 0, stream, (const float *)d_pur, n, batch, d_out,
                     d_purities);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

// below the tile size: one (cache-resident) sweep per wire
int mw_run_sweeps(const float2 *states, int n, int batch, float *d_out, float *d_purities, char *ws, const MwLayout &L,
                  hipStream_t stream) {
  const int nb = overlap_blocks(n);
  float4 *partial = (float4 *)(ws + L.partial.off);
  for (int p = 0; p < n; ++p)
    hipLaunchKernelGGL(k_cross_partial, dim3(nb, batch), dim3(256), 0, stream, (const float4 *)states, n, p, partial, nb);
  hipLaunchKernelGGL(k_mw_final, dim3(batch), dim3(nb >= 256 ? 256 : 64), 0, stream, (const float4 *)partial, n, nb,
                     batch, d_out, d_purities);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

// The stand-alone route, shared by its two entries: arguments, reads, layout, the one workspace check, the run.
// packed: Q and the purities by wire go to the layout's packed regions (run_mw_resident packs them afterwards).
int mw_standalone(const void *states, int n, int batch, float *d_out, float *d_purities, void *ws_, size_t ws_bytes,
                  bool packed, hipStream_t stream, MwLayout *layout = nullptr) {
  if (!states || !ws_ || n < 1 || n > QMLE_MAX_QUBITS || batch < 1 || batch > kMaxGridY) return QMLE_ERR_INVALID_ARG;
  const MwReads rd = n >= kMwT ? mw_reads_standalone(n, batch) : MwReads{};
  if (!rd.ok) return QMLE_ERR_INTERNAL;
  const MwLayout L = mw_layout_standalone(n, batch, rd, packed);
  if (ws_bytes < L.end) return QMLE_ERR_WORKSPACE;
  if (layout) *layout = L;
  char *ws = (char *)ws_;
  if (packed) {
    d_out = (float *)(ws + L.packed_q.off);
    d_purities = (float *)(ws + L.packed_pur.off);
  }
  return n >= kMwT ? mw_run_tiled((const float2 *)states, n, batch, d_out, d_purities, ws, rd, L, stream)
                   : mw_run_sweeps((const float2 *)states, n, batch, d_out, d_purities, ws, L, stream);
}

// what the finish kernels of a fused call read: where a position sits in the producing tile or the tile index, and
// the rows of the later reads
MwFusedArgs mw_fused_args(int n, const Stage &last, int row_shift, bool lean, const MwReads &rd, const MwLayout &L,
                          char *ws) {
  MwFusedArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  pa.first = (const float *)(ws + L.first.off);
  pa.rows_first = (1u << (n - last.T)) >> row_shift;
  pa.lg = row_shift;
  pa.T = last.T;
  pa.n = n;
  pa.lean = lean ? 1 : 0;
  for (int p = 0; p < QMLE_MAX_QUBITS; ++p) {
    pa.loc[p] = pa.outer_idx[p] = -1;
    pa.src_read[p] = (int8_t)rd.src_read[p];  // (kMwFromFirst is the kernels' -1)
    pa.src_col[p] = (int8_t)rd.src_col[p];
  }
  for (int j = 0; j < last.T; ++j) pa.loc[(int)last.tile_bits[j]] = (int8_t)j;
  for (int i = 0; i < n - last.T; ++i) pa.outer_idx[(int)last.outer_bits[i]] = (int8_t)i;
  for (int r = 0; r < rd.n_later; ++r) {
    pa.later[r] = (const float *)(ws + L.later[r].off);
    pa.rows_later[r] = rd.rows[r];
    pa.later_stride[r] = (uint32_t)rd.stride[r];
  }
  return pa;
}

int mw_finish_columns(const MwFusedArgs &pa, int batch, int n_later, const MwLayout &L, char *ws, float *d_out,
                      hipStream_t stream) {
  MwColsumArgs ca;
  std::memset(&ca, 0, sizeof(ca));
  ca.slices = L.slices;
  ca.rows[0] = pa.first; ca.n_rows[0] = pa.rows_first; ca.stride[0] = kMwFusedRowA; ca.n_cols[0] = kMwFusedRowA;
  ca.tot_col = 3 * pa.T;
  ca.n_signed = pa.n - pa.T - pa.lg > 0 ? pa.n - pa.T - pa.lg : 0;
  for (int r = 0; r < n_later; ++r) {
    ca.rows[1 + r] = pa.later[r]; ca.n_rows[1 + r] = pa.rows_later[r]; ca.stride[1 + r] = pa.later_stride[r];
    ca.n_cols[1 + r] = (int)pa.later_stride[r];
  }
  const int n_mats = 1 + n_later;
  for (int m = 0; m < n_mats; ++m) ca.out[m] = (double *)(ws + L.colsum[m].off);
  hipLaunchKernelGGL(k_mw_colsum, dim3(L.slices, batch, n_mats), dim3(L.finish_threads), 0, stream, ca);
  hipLaunchKernelGGL(k_mw_finish_cols, dim3(batch), dim3(1024), 0, stream, pa, ca, n_mats, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int mw_finish_per_position(const MwFusedArgs &pa, int batch, const MwLayout &L, char *ws, float *d_out,
                           hipStream_t stream) {
  const int n = pa.n, slices = L.slices;
  float *d_pur = (float *)(ws + L.pur.off);
  double *d_part = (double *)(ws + L.partial.off);
  hipLaunchKernelGGL(k_mw_purity_fused, dim3(batch, n, slices), dim3(L.finish_threads), 0, stream, pa, d_pur, d_part);
  if (slices > 1)
    hipLaunchKernelGGL(k_mw_purity_final, dim3((batch * n + 63) / 64), dim3(64), 0, stream, (const double *)d_part, n,
                       batch, slices, d_pur);
  hipLaunchKernelGGL(k_mw_pack, dim3((batch + 63) / 64), dim3(64), 0, stream, (const float *)d_pur, n, batch, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

// ---- the description (qmle_meyer_wallach_describe) ----
void js_add(std::string &js, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void js_add(std::string &js, const char *fmt, ...) {
  char tmp[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(tmp, sizeof(tmp), fmt, ap);
  va_end(ap);
  js += tmp;
}
void js_read(std::string &js, MwReadKind kind, int lo, int lo2, int q, uint32_t rows, int stride, bool nt) {
  js_add(js, "{\"kind\":\"%s\",\"lo\":%d,\"lo2\":%d,\"q\":%d,\"rows\":%u,\"stride\":%d,\"nt\":%s}", kMwReadKindNames[kind],
         lo, lo2, q, rows, stride, nt ? "true" : "false");
}
void js_region(std::string &js, const char *name, int idx, const MwRegion &r, bool doubles, bool &any) {
  js += any ? "," : "";
  any = true;
  if (idx < 0) js_add(js, "{\"name\":\"%s\"", name);
  else js_add(js, "{\"name\":\"%s%d\"", name, idx);
  js_add(js, ",\"offset\":%zu,\"bytes\":%zu,\"doubles\":%s}", r.off, r.bytes, doubles ? "true" : "false");
}
// "first": the stand-alone first read, or null; "reads": the later reads; "positions"[p]: later read (-1: the
// first read / the producing pass) and column; "regions": what the run places where
std::string mw_describe(const char *route, int n, int batch, bool fusable, bool lean, bool tiled_standalone,
                        const MwReads &rd, const MwLayout &L, const char *finish) {
  const bool nt = launch_streams_past_caches((uint64_t)batch, n);
  std::string js;
  js_add(js, "{\"route\":\"%s\",\"n\":%d,\"batch\":%d,\"fusable\":%s,\"lean\":%s,\"first\":", route, n, batch,
         fusable ? "true" : "false", lean ? "true" : "false");
  if (tiled_standalone) js_read(js, kMwReadFirst, 4, 8, rd.q_first, rd.rows_first, kMwRowFirst, nt);
  else js += "null";
  js += ",\"reads\":[";
  for (int r = 0; r < rd.n_later; ++r) {
    js += r ? "," : "";
    js_read(js, rd.stride[r] == kMwRowLaterLow ? kMwReadLaterLow : kMwReadLater, rd.lo[r], rd.lo2[r], rd.q[r], rd.rows[r],
            rd.stride[r], nt);
  }
  js += "],\"positions\":[";
  for (int p = 0; p < n; ++p) js_add(js, "%s{\"read\":%d,\"col\":%d}", p ? "," : "", rd.src_read[p], rd.src_col[p]);
  js_add(js, "],\"finish\":\"%s\",\"slices\":%d,\"finish_threads\":%d,\"regions\":[", finish, L.slices, L.finish_threads);
  bool any = false;
  if (L.first.bytes) js_region(js, "first", -1, L.first, false, any);
  for (int r = 0; r < rd.n_later; ++r) js_region(js, "later", r, L.later[r], false, any);
  if (L.pur.bytes) js_region(js, "purities", -1, L.pur, false, any);
  if (L.partial.bytes) js_region(js, "partial", -1, L.partial, L.first.bytes != 0, any);
  for (int m = 0; m <= kMwMaxLater; ++m)
    if (L.colsum[m].bytes) js_region(js, "colsum", m, L.colsum[m], true, any);
  if (L.packed_q.bytes) js_region(js, "packed_q", -1, L.packed_q, false, any);
  if (L.packed_pur.bytes) js_region(js, "packed_purities", -1, L.packed_pur, false, any);
  js_add(js, "],\"end\":%zu,\"total_bytes\":%zu}", L.end, L.total);
  return js;
}

}  // namespace

namespace qmle {

// Can stage `last` (the plan's last one) report its tile's Meyer-Wallach sums, and do fewer reads
// than the stand-alone kernel's remain?  (16 amplitudes per work item: T >= 10.)
bool mw_fusable(int n, const Stage &last) {
  if (last.kind != ST_TILE || last.T < 10 || last.T > 14) return false;
  if (last.T == n) return true;
  const MwReads rd = mw_reads_fused(n, 1, last, false);
  return rd.ok && rd.n_later < qmle_meyer_wallach_reads(n);
}

// Tiled state: positions 0..3 sit in the producing tile AND in the tile of every later read; the later reads are
// bound by HBM, the producing pass by its arithmetic -- so the first later read reports them (QMLE_MW_NO_LEAN=1: A/B).
bool mw_no_lean_switch() { return std::getenv("QMLE_MW_NO_LEAN") != nullptr; }  // (read per call)
bool mw_lean(int n, const Stage &last) { return mw_lean_layout(n, last) && !mw_no_lean_switch(); }
bool mw_lean_layout(int n, const Stage &last) {
  if (last.kind != ST_TILE || last.T >= n || last.T < 10) return false;
  for (int j = 0; j < 4; ++j)
    if (last.tile_bits[j] != j) return false;
  const MwReads rd = mw_reads_fused(n, 1, last, false);
  return rd.ok && rd.n_later >= 1;
}

// A tiled state takes the per-position finish whatever its shape (QMLE_MW_FINISH_PER_POSITION=1: the tests of that
// finish at sizes whose own finish is the columns one).  Read per call; the workspace holds either finish.
static bool mw_per_position_switch() { return std::getenv("QMLE_MW_FINISH_PER_POSITION") != nullptr; }

size_t mw_fused_ws_bytes(int n, int batch, const Stage &last) {
  return mw_layout_fused(n, batch, mw_reads_fused(n, batch, last, false), last.T, 0, false).total;
}

// rows_first = ws (filled by the producing pass: [batch][tiles][kMwFusedRowA]); the later reads' rows and
// the finish's regions follow it.  d_out [batch][n + 1] = (Q, purities by wire).  *finish_run: the finish it queued.
int run_mw_fused(const float2 *states, int n, int batch, const Stage &last, int row_shift, void *ws_,
                 size_t ws_bytes, float *d_out, hipStream_t stream, int *finish_run) {
  if (batch < 1 || batch > kMaxGridY) return QMLE_ERR_INVALID_ARG;
  const bool lean = last.T < n && mw_lean(n, last);
  const MwReads rd = mw_reads_fused(n, batch, last, lean);
  if (!rd.ok) return QMLE_ERR_INTERNAL;
  const MwLayout L = mw_layout_fused(n, batch, rd, last.T, row_shift, mw_per_position_switch());
  if (ws_bytes < L.end) return QMLE_ERR_WORKSPACE;
  char *ws = (char *)ws_;
  const MwFusedArgs pa = mw_fused_args(n, last, row_shift, lean, rd, L, ws);
  const int rc = mw_issue_later_reads(states, n, batch, rd, L, ws, stream);
  if (rc != QMLE_OK) return rc;
  if (finish_run) *finish_run = L.finish;
  switch (L.finish) {
    case kMwFinishWholeState:
      hipLaunchKernelGGL(k_mw_whole_state_finish, dim3((batch + L.finish_threads - 1) / L.finish_threads),
                         dim3(L.finish_threads), 0, stream, pa, batch, d_out);
      HIPCHK(hipGetLastError());
      return QMLE_OK;
    case kMwFinishColumns: return mw_finish_columns(pa, batch, rd.n_later, L, ws, d_out, stream);
    default: return mw_finish_per_position(pa, batch, L, ws, d_out, stream);
  }
}

// resident states, no producing pass to lean on: the stand-alone route, packed like run_mw_fused
int run_mw_resident(const float2 *states, int n, int batch, void *ws, size_t ws_bytes, float *d_out,
                    hipStream_t stream) {
  if (!d_out) return QMLE_ERR_INVALID_ARG;
  MwLayout L;
  const int rc = mw_standalone(states, n, batch, nullptr, nullptr, ws, ws_bytes, /*packed=*/true, stream, &L);
  if (rc != QMLE_OK) return rc;
  hipLaunchKernelGGL(k_mw_pack_wires, dim3((batch + 63) / 64), dim3(64), 0, stream,
                     (const float *)((char *)ws + L.packed_q.off), (const float *)((char *)ws + L.packed_pur.off), n,
                     batch, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

size_t mw_resident_ws_bytes(int n, int batch) {
  return mw_layout_standalone(n, batch, n >= kMwT ? mw_reads_standalone(n, batch) : MwReads{}, true).total;
}

}  // namespace qmle

extern "C" {

int qmle_meyer_wallach_reads(int n_qubits) {
  if (n_qubits < 1 || n_qubits > QMLE_MAX_QUBITS) return 0;
  // below the tile size: one (cache-resident) sweep per wire
  return n_qubits >= kMwT ? 1 + mw_reads_standalone(n_qubits, 1).n_later : n_qubits;
}

size_t qmle_meyer_wallach_workspace_bytes(int n_qubits, int batch) {
  if (n_qubits < 1 || batch < 1) return 0;
  return mw_layout_standalone(n_qubits, batch, n_qubits >= kMwT ? mw_reads_standalone(n_qubits, batch) : MwReads{}, false)
      .total;
}

int qmle_meyer_wallach(const void *d_states, int n_qubits, int batch, float *d_out, float *d_purities,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream_) {
  if (!d_out) return QMLE_ERR_INVALID_ARG;
  return mw_standalone(d_states, n_qubits, batch, d_out, d_purities, d_workspace, workspace_bytes, /*packed=*/false,
                       (hipStream_t)stream_);
}

int qmle_meyer_wallach_describe(const qmle_plan *plan, int n_qubits, int batch, int row_shift, unsigned request_flags,
                                char *buf, size_t cap) {
  using namespace qmle;
  const qmle_plan *exec = plan ? qmle_plan_executed(const_cast<qmle_plan *>(plan), QMLE_MEAS_MEYER_WALLACH) : nullptr;
  if (plan && !exec) exec = plan;
  const int n = exec ? exec->n : n_qubits;
  if (n < 1 || n > QMLE_MAX_QUBITS || batch < 1 || batch > kMaxGridY || row_shift < 0) return QMLE_ERR_INVALID_ARG;
  std::string js;
  const Stage *last = exec && !exec->stages.empty() ? &exec->stages.back() : nullptr;
  if (last && mw_fusable(n, *last)) {
    if (row_shift > n - last->T) return QMLE_ERR_INVALID_ARG;
    const bool lean = mw_lean_layout(n, *last) && !(request_flags & QMLE_ROUTE_NO_MW_LEAN);
    const MwReads rd = mw_reads_fused(n, batch, *last, lean);
    const MwLayout L = mw_layout_fused(n, batch, rd, last->T, row_shift, request_flags & QMLE_ROUTE_MW_PER_POSITION);
    js = mw_describe("fused", n, batch, true, lean, false, rd, L, kMwFinishNames[L.finish]);
  } else {
    const MwReads rd = n >= kMwT ? mw_reads_standalone(n, batch) : MwReads{};
    const MwLayout L = mw_layout_standalone(n, batch, rd, /*packed=*/plan != nullptr);
    js = mw_describe(plan ? "resident" : "standalone", n, batch, false, false, n >= kMwT, rd, L,
                     n >= kMwT ? "standalone" : "per-wire-sweeps");
  }
  if (buf && cap > 0) {
    const size_t nc = js.size() < cap - 1 ? js.size() : cap - 1;
    std::memcpy(buf, js.data(), nc);
    buf[nc] = 0;
  }
  return (int)js.size();
}

}  // extern "C"
