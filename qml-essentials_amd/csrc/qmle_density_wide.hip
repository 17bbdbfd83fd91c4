// libqmle_sv, Kraus maps on three or four system wires of a resident vec(rho) (qmle_density_apply_wide):
// rho -> sum_m K_m rho K_m^+ in place, one read and one write of vec(rho), on the matrix cores, both precisions.
// With one unitary K it is a wide gate on a noisy tape, with a Kraus set a wide channel.
//
// The tile.  vec(rho) is a register of 2n bit positions; wire w has its ket bit on position 2n - 1 - w and its bra
// bit on n - 1 - w.  A workgroup stages a tile of up to 12 positions in LDS: the 2k target positions and the lowest
// non-target positions.  Positions 0..3 are then always tile positions, so a thread's neighbours in the workgroup
// read and write 16 consecutive amplitudes: whole 128-byte lines (256 bytes in complex128), whatever the wires are.
// For fixed non-target bits the 4^k amplitudes on the target positions are a d x d block R (d = 2^k), row = the ket
// bits, column = the bra bits, both in ASCENDING order of their positions; the operators are permuted to that
// order when they are fetched (pbit), so every wire order runs the same code.  A register smaller than the tile
// leaves the rest of the 4096 LDS slots zero: the instructions run on whole tiles whatever n is.
//
// Matrix instructions.  v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 compute D += A B with the operand layout
// of qmle_wide.hip: a lane (g = lane >> 4, c = lane & 15) supplies A[i = c][kk = g] and B[kk = g][j = c], and its
// accumulator register r holds D[row(g, r)][c], row = 4 g + r in float32 and g + 4 r in float64.  A complex product
// is four real ones.
//
// Sandwich form (k_dwide_sandwich): R' = sum_m K_m R K_m^+.  The LDS tile is [non-target bits][ket][bra], so a block
// is 4^k consecutive slots.  Per operator two products:
//   first   P = A1 B1, A1[i][kk] = R[kk][i], B1[kk][j] = K[j][kk]:  P[i][j] = (K R)[j][i] = T[j][i], T = K R.
//   second  R' += A2 B2 with A2[i][m] = T[i][m], B2[m][j] = conj(K[j][m]).
// The layout argument: the lane (g, c) holds P[row(g, r)][c] = T[c][row(g, r)] in accumulator register r, and that
// is exactly what it must supply as A2[i = c][m] when step r of the second product visits the contraction indices
// m = row(g, r), g = 0..3.  Over r = 0..3 these are all sixteen m once each -- the contraction index may be visited
// in any order -- so the first product's accumulators feed the second one without leaving their registers; only the
// constant operand is fetched in that order (B2[m = row(g, r)][j = c], offsets o2).  The result lands as
// R'[row(g, r)][c], the layout of the block in LDS.  For d = 8 two blocks share the sixteen rows and columns (block
// h = c >> 3): the first product contracts eight indices (two steps) and computes the two wanted 8x8 products in its
// diagonal blocks; in the second one B2[m][j] is zero where m and j belong to different blocks, which removes the
// other block's T from the sum, and only the two diagonal 8x8 results are stored (as k_wide_moment keeps them).
//
// Superoperator form (k_dwide_super): vec(R') = S vec(R), S = sum_m K_m (x) conj(K_m) (d^2 x d^2, built in float64
// in a fixed order by k_dwide_build_super, rounded once to the run's precision).  The LDS tile is
// [ket][bra][non-target bits]: X[kk][block], a d^2 x 4096 / d^2 matrix, and the pass is the GEMM S X: 16 output
// tiles of 16x16, four per wave, d^2 / 4 contraction steps.  S lies in the workspace in the order the lanes fetch
// it ([row tile][step][lane]: one 512-byte line per wave and step), permuted to ascending positions, and is read
// through L1 / L2: 32 KiB (k = 3) or 512 KiB (k = 4) in complex64.
//
// Control flow around the matrix instructions is wave-uniform (loops over operators, steps and blocks with uniform
// bounds); no atomics, a fixed summation order: the same bits from call to call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "qmle_internal.h"
#include "qmle_host.h"
#include "qmle_dev.h"

namespace {

typedef float dw_f4 __attribute__((ext_vector_type(4)));
typedef double dw_d4 __attribute__((ext_vector_type(4)));

constexpr int kDwTileBits = 12, kDwTile = 1 << kDwTileBits, kDwThreads = 256;

struct DwTile {
  int tb;                   // real tile positions (min(12, 2n)); tile bits tb..11 are virtual: zeros in LDS
  int tp[kDwTileBits];      // tile bit i sits on position tp[i] of the register (ascending; tp[i] = i for i < 4)
  int lb[kDwTileBits];      // ... and on bit lb[i] of the LDS slot
  int pbit[4];              // bit q of a block's row / column index is bit pbit[q] of the caller's matrix index
};

__device__ __forceinline__ dw_f4 dw_mfma(float a, float b, dw_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ dw_d4 dw_mfma(double a, double b, dw_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
// acc += a b, complex
template <class T, class ACC>
__device__ __forceinline__ void dw_cmac(T ar, T ai, T br, T bi, ACC &re, ACC &im) {
  re = dw_mfma(ar, br, re);
  re = dw_mfma(-ai, bi, re);
  im = dw_mfma(ar, bi, im);
  im = dw_mfma(ai, br, im);
}
template <bool F64> __device__ __forceinline__ int dw_row(int g, int r) { return F64 ? g + 4 * r : 4 * g + r; }

// the caller's matrix index of the block index a (ascending positions)
template <int K> __device__ __forceinline__ int dw_perm(int a, const DwTile &W) {
  int o = 0;
#pragma unroll
  for (int q = 0; q < K; ++q) o |= ((a >> q) & 1) << W.pbit[q];
  return o;
}

// Tile <-> register.  Thread t of 256 takes the tile-local indices t + 256 j: their low 8 bits are the thread's,
// so the offsets split into a per-thread part and a per-j part.
struct DwMap {
  uint64_t g_lo;  // register offset of the thread's low 8 tile bits
  int l_lo;       // LDS slot bits of the same
};
__device__ __forceinline__ DwMap dw_map_lo(const DwTile &W) {
  DwMap m{0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int b = (threadIdx.x >> i) & 1;
    m.g_lo |= (uint64_t)b << W.tp[i];
    m.l_lo |= b << W.lb[i];
  }
  return m;
}
__device__ __forceinline__ uint64_t dw_tile_base(const DwTile &W) {  // the workgroup's tile: blockIdx.x on the other positions
  uint64_t base = blockIdx.x;
  for (int i = 0; i < W.tb; ++i) base = ins0_64(base, W.tp[i]);
  return base;
}
template <class V> __device__ __forceinline__ void dw_load_tile(const V *__restrict__ rho, const DwTile &W, const DwMap &m, V *tile) {
#pragma unroll
  for (int j = 0; j < kDwTile / kDwThreads; ++j) {
    uint64_t g = m.g_lo;
    int l = m.l_lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      g |= (uint64_t)((j >> i) & 1) << W.tp[8 + i];
      l |= ((j >> i) & 1) << W.lb[8 + i];
    }
    V v;
    v.x = 0, v.y = 0;
    if ((int)(threadIdx.x + kDwThreads * j) < (1 << W.tb)) v = rho[g];
    tile[l] = v;
  }
}
template <class V> __device__ __forceinline__ void dw_store_tile(V *__restrict__ rho, const DwTile &W, const DwMap &m, const V *tile) {
#pragma unroll
  for (int j = 0; j < kDwTile / kDwThreads; ++j) {
    uint64_t g = m.g_lo;
    int l = m.l_lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      g |= (uint64_t)((j >> i) & 1) << W.tp[8 + i];
      l |= ((j >> i) & 1) << W.lb[8 + i];
    }
    if ((int)(threadIdx.x + kDwThreads * j) < (1 << W.tb)) rho[g] = tile[l];
  }
}

template <int K, bool F64>
__global__ void __launch_bounds__(kDwThreads)
k_dwide_sandwich(void *__restrict__ rho_all, int n2, const DwTile W, const double2 *__restrict__ ops, int n_ops, int per_sample) {
  constexpr int D = 1 << K, DD = D * D, S1 = D / 4, PAIR = 16 / D, UNIT = DD * PAIR, UNITS = kDwTile / UNIT;
  using V = std::conditional_t<F64, double2, float2>;
  using T = std::conditional_t<F64, double, float>;
  using ACC = std::conditional_t<F64, dw_d4, dw_f4>;
  __shared__ V tile[kDwTile];
  V *__restrict__ rho = (V *)rho_all + ((uint64_t)blockIdx.y << n2) + dw_tile_base(W);
  if (per_sample) ops += (size_t)blockIdx.y * DD;
  const DwMap map = dw_map_lo(W);
  dw_load_tile(rho, W, map, tile);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, g = lane >> 4, c = lane & 15;
  const int cb = c & (D - 1), half = c >> K;  // (D = 16: half = 0)
  int o1[S1], o2[4];
  bool keep[4];
  const int prow = dw_perm<K>(cb, W) * D;
#pragma unroll
  for (int s = 0; s < S1; ++s) o1[s] = prow + dw_perm<K>(4 * s + g, W);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = dw_row<F64>(g, r);
    o2[r] = prow + dw_perm<K>(m & (D - 1), W);
    keep[r] = (m >> K) == half;  // (D = 16: always)
  }
  __syncthreads();
  for (int u = wv; u < UNITS; u += kDwThreads / kWave) {  // (wave-uniform)
    V *blk = tile + u * UNIT + half * DD;
    T ar[S1], ai[S1];
#pragma unroll
    for (int s = 0; s < S1; ++s) {
      const V v = blk[(4 * s + g) * D + cb];
      ar[s] = v.x, ai[s] = v.y;
    }
    ACC rre = {0, 0, 0, 0}, rim = {0, 0, 0, 0};
    for (int m = 0; m < n_ops; ++m) {  // (wave-uniform)
      const double2 *__restrict__ km = ops + (size_t)m * DD;
      ACC pre = {0, 0, 0, 0}, pim = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < S1; ++s) {
        const double2 b = km[o1[s]];
        dw_cmac<T, ACC>(ar[s], ai[s], (T)b.x, (T)b.y, pre, pim);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double2 b = km[o2[r]];
        const T br = keep[r] ? (T)b.x : (T)0, bi = keep[r] ? (T)-b.y : (T)0;  // conj(K), zero across the two blocks
        dw_cmac<T, ACC>(pre[r], pim[r], br, bi, rre, rim);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = dw_row<F64>(g, r);
      if ((row >> K) == half) {
        V v;
        v.x = rre[r], v.y = rim[r];
        blk[(row & (D - 1)) * D + cb] = v;
      }
    }
  }
  __syncthreads();
  dw_store_tile(rho, W, map, tile);
}

// sfrag[(rt * STEPS + s) * 64 + lane] = S[16 rt + (lane & 15)][4 s + (lane >> 4)] in ascending-position order:
// S[(a, b), (c, e)] = sum_m K_m[a][c] conj(K_m[b][e]), added in float64 in the order of m
template <int K, class V>
__global__ void __launch_bounds__(256)
k_dwide_build_super(const double2 *__restrict__ ops, int n_ops, const DwTile W, V *__restrict__ sfrag) {
  constexpr int D = 1 << K, DD = D * D, STEPS = DD / 4;
  const int e_ = blockIdx.x * 256 + threadIdx.x;
  if (e_ >= DD * DD) return;
  const int lane = e_ & 63, s = (e_ >> 6) % STEPS, rt = (e_ >> 6) / STEPS;
  const int row = 16 * rt + (lane & 15), col = 4 * s + (lane >> 4);
  const int ia = dw_perm<K>(row / D, W) * D + dw_perm<K>(col / D, W), ib = dw_perm<K>(row % D, W) * D + dw_perm<K>(col % D, W);
  double sr = 0.0, si = 0.0;
  for (int m = 0; m < n_ops; ++m) {
    const double2 a = ops[(size_t)m * DD + ia], b = ops[(size_t)m * DD + ib];
    sr += a.x * b.x + a.y * b.y;  // a conj(b)
    si += a.y * b.x - a.x * b.y;
  }
  V v;
  v.x = sr, v.y = si;
  sfrag[e_] = v;
}

template <int K, bool F64>
__global__ void __launch_bounds__(kDwThreads)
k_dwide_super(void *__restrict__ rho_all, int n2, const DwTile W, const void *__restrict__ sfrag_) {
  constexpr int DD = 1 << (2 * K), NB = kDwTile / DD, STEPS = DD / 4, Q = 4;  // Q row tiles per wave
  using V = std::conditional_t<F64, double2, float2>;
  using T = std::conditional_t<F64, double, float>;
  using ACC = std::conditional_t<F64, dw_d4, dw_f4>;
  __shared__ V tile[kDwTile];
  V *__restrict__ rho = (V *)rho_all + ((uint64_t)blockIdx.y << n2) + dw_tile_base(W);
  const V *__restrict__ sfrag = (const V *)sfrag_;
  const DwMap map = dw_map_lo(W);
  dw_load_tile(rho, W, map, tile);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, g = lane >> 4, c = lane & 15;
  // k = 3: 4 column tiles (one per wave) x 4 row tiles; k = 4: 1 column tile x 16 row tiles (four per wave)
  const int ct = K == 3 ? wv : 0, rt0 = K == 3 ? 0 : Q * wv;
  ACC re[Q], im[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) re[q] = ACC{0, 0, 0, 0}, im[q] = ACC{0, 0, 0, 0};
  __syncthreads();
#pragma unroll 2
  for (int s = 0; s < STEPS; ++s) {
    const V b = tile[(4 * s + g) * NB + 16 * ct + c];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const V a = sfrag[((size_t)(rt0 + q) * STEPS + s) * kWave + lane];
      dw_cmac<T, ACC>(a.x, a.y, b.x, b.y, re[q], im[q]);
    }
  }
  __syncthreads();  // every wave has read X before anyone overwrites it
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      V v;
      v.x = re[q][r], v.y = im[q][r];
      tile[(16 * (rt0 + q) + dw_row<F64>(g, r)) * NB + 16 * ct + c] = v;
    }
  __syncthreads();
  dw_store_tile(rho, W, map, tile);
}

constexpr int kFormAuto = 0, kFormSandwich = 1, kFormSuper = 2;

// Arithmetic of the two forms per amplitude: 2 d n_ops (sandwich) against d^2 (superoperator), level at n_ops = d / 2.
// The measured times cross earlier (profiles/density_wide.md, leg 3: the sandwich fetches its operators per block, the
// superoperator pass costs the same whatever n_ops is): at k = 3 the superoperator is ahead from two operators on, at
// k = 4 the sandwich wins at 4 operators and loses at 8.  The automatic rule follows the measurement: the sandwich for
// one operator per sample (no shared S), for a single operator at k = 3 and for up to four at k = 4.
int dw_auto_form(int k, int n_ops, int per_sample) { return per_sample || n_ops <= (k == 3 ? 1 : 4) ? kFormSandwich : kFormSuper; }

// everything the call refuses that the workspace query can see; form resolved
int dw_check(int n_qubits, int batch, int k, int n_ops, int f64, int per_sample, int &form) {
  if (k != 3 && k != 4) return QMLE_ERR_UNSUPPORTED;
  if (batch < 1 || n_qubits < k || 2 * n_qubits > QMLE_MAX_QUBITS || (f64 != 0 && f64 != 1) || (per_sample != 0 && per_sample != 1) ||
      form < kFormAuto || form > kFormSuper || n_ops < 1 || (per_sample && (n_ops != 1 || form == kFormSuper)) ||
      (form == kFormSandwich && n_ops > (1 << (2 * k))))
    return QMLE_ERR_INVALID_ARG;
  if (form == kFormAuto) form = dw_auto_form(k, n_ops, per_sample);
  return QMLE_OK;
}
size_t dw_ws_bytes(int k, int f64, int form) {  // (256 bytes for aligning it)
  return (form == kFormSuper ? ((size_t)1 << (4 * k)) * (f64 ? sizeof(double2) : sizeof(float2)) : 0) + 256;
}

template <int K, bool F64>
int dw_launch(int form, dim3 grid, hipStream_t stream, void *rho, int n2, const DwTile &W, const double2 *ops, int n_ops,
              int per_sample, void *sfrag) {
  if (form == kFormSandwich) hipLaunchKernelGGL((k_dwide_sandwich<K, F64>), grid, dim3(kDwThreads), 0, stream, rho, n2, W, ops, n_ops, per_sample);
  else hipLaunchKernelGGL((k_dwide_super<K, F64>), grid, dim3(kDwThreads), 0, stream, rho, n2, W, (const void *)sfrag);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

}  // namespace

extern "C" {

int qmle_density_apply_wide_form(int k, int n_ops, int per_sample) {
  if (k != 3 && k != 4) return QMLE_ERR_UNSUPPORTED;
  if (n_ops < 1 || (per_sample != 0 && per_sample != 1) || (per_sample && n_ops != 1)) return QMLE_ERR_INVALID_ARG;
  return dw_auto_form(k, n_ops, per_sample);
}

size_t qmle_density_apply_wide_workspace_bytes(int n_qubits, int batch, int k, int n_ops, int f64, int form) {
  if (dw_check(n_qubits, batch, k, n_ops, f64, 0, form) != QMLE_OK) return 0;
  return dw_ws_bytes(k, f64, form);
}

int qmle_density_apply_wide(void *d_rho, int n_qubits, int batch, int f64, const int32_t *wires, int k, const void *d_ops,
                            int n_ops, int per_sample, int form, void *d_ws, size_t ws_bytes, qmle_stream stream_) {
  if (k != 3 && k != 4) return QMLE_ERR_UNSUPPORTED;
  if (!d_rho || !wires || !d_ops || !d_ws) return QMLE_ERR_INVALID_ARG;
  const int rc = dw_check(n_qubits, batch, k, n_ops, f64, per_sample, form);
  if (rc != QMLE_OK) return rc;
  for (int i = 0; i < k; ++i)
    if (wires[i] < 0 || wires[i] >= n_qubits) return QMLE_ERR_WIRE_RANGE;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < i; ++j)
      if (wires[i] == wires[j]) return QMLE_ERR_DUPLICATE_WIRES;
  char *ws = (char *)d_ws;
  if (ws_bytes < dw_ws_bytes(k, f64, form) || !align_workspace(ws, ws_bytes)) return QMLE_ERR_WORKSPACE;

  // the tile: bra positions n - 1 - w and ket positions 2n - 1 - w of the wires, then the lowest other positions
  const int n = n_qubits, n2 = 2 * n, tb = std::min(kDwTileBits, n2), nt = kDwTileBits - 2 * k;
  DwTile W{};
  W.tb = tb;
  uint32_t target = 0;
  for (int i = 0; i < k; ++i) target |= (1u << (n - 1 - wires[i])) | (1u << (n2 - 1 - wires[i]));
  uint32_t in_tile = target;
  for (int p = 0, free_ = tb - 2 * k; p < n2 && free_ > 0; ++p)
    if (!(in_tile & (1u << p))) in_tile |= 1u << p, --free_;
  // LDS bits: sandwich [non-targets][ket][bra] -- targets on bits 0.., non-targets above; superoperator
  // [ket][bra][non-targets] -- non-targets on bits 0.., targets above.  Virtual tile bits count as non-targets.
  int ti = 0, lt = form == kFormSandwich ? 0 : nt, ln = form == kFormSandwich ? 2 * k : 0;
  for (int p = 0; p < n2; ++p)
    if (in_tile & (1u << p)) {
      W.tp[ti] = p;
      W.lb[ti] = (target & (1u << p)) ? lt++ : ln++;
      ++ti;
    }
  for (; ti < kDwTileBits; ++ti) W.tp[ti] = 0, W.lb[ti] = ln++;
  // bit q of a block index: the q-th lowest bra position = n - 1 - wire; wire i is bit k - 1 - i of the caller's index
  for (int q = 0, p = 0; p < n; ++p)
    if (target & (1u << p)) {
      for (int i = 0; i < k; ++i)
        if (n - 1 - wires[i] == p) W.pbit[q] = k - 1 - i;
      ++q;
    }

  hipStream_t stream = (hipStream_t)stream_;
  const size_t amp = f64 ? sizeof(double2) : sizeof(float2), dd = (size_t)1 << (2 * k);
  const double2 *ops = (const double2 *)d_ops;
  if (form == kFormSuper) {
    const dim3 bgrid((unsigned)(dd * dd / 256));
    if (k == 3) {
      if (f64) hipLaunchKernelGGL((k_dwide_build_super<3, double2>), bgrid, dim3(256), 0, stream, ops, n_ops, W, (double2 *)ws);
      else hipLaunchKernelGGL((k_dwide_build_super<3, float2>), bgrid, dim3(256), 0, stream, ops, n_ops, W, (float2 *)ws);
    } else {
      if (f64) hipLaunchKernelGGL((k_dwide_build_super<4, double2>), bgrid, dim3(256), 0, stream, ops, n_ops, W, (double2 *)ws);
      else hipLaunchKernelGGL((k_dwide_build_super<4, float2>), bgrid, dim3(256), 0, stream, ops, n_ops, W, (float2 *)ws);
    }
    HIPCHK(hipGetLastError());
  }
  const unsigned tiles = 1u << (n2 - tb);
  for (int b0 = 0; b0 < batch; b0 += kMaxGridY) {
    const int nbatch = std::min(kMaxGridY, batch - b0);
    void *rho = (char *)d_rho + ((size_t)b0 << n2) * amp;
    const double2 *o = ops + (per_sample ? (size_t)b0 * dd : 0);
    const dim3 grid(tiles, (unsigned)nbatch);
    int lrc;
    if (k == 3) lrc = f64 ? dw_launch<3, true>(form, grid, stream, rho, n2, W, o, n_ops, per_sample, ws)
                          : dw_launch<3, false>(form, grid, stream, rho, n2, W, o, n_ops, per_sample, ws);
    else lrc = f64 ? dw_launch<4, true>(form, grid, stream, rho, n2, W, o, n_ops, per_sample, ws)
                   : dw_launch<4, false>(form, grid, stream, rho, n2, W, o, n_ops, per_sample, ws);
    if (lrc != QMLE_OK) return lrc;
  }
  return QMLE_OK;
}

}  // extern "C"
