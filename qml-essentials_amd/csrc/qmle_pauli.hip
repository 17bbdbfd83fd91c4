// libqmle_sv, Pauli-word observables of resident states: qmle_expval_pauli (complex64), its complex128
// twin and qmle_density_expval_pauli; qmle_apply_pauli_sum and the seed of the adjoint sweep.  Every X / Y / Hermitian observable is a real-weighted sum of
// words P = i^ny X^x Z^z, and
//   <psi|P|psi> = Re[(-i)^ny S],   S = sum_i conj(psi_i) (-1)^popc(i & z) psi_{i ^ x}
// needs every amplitude and its partner i ^ x once.  (The sign is taken at the row index i; the
// definition's sign at the partner index differs by (-1)^popc(x & z) = (-1)^ny, which turns i^ny into
// (-i)^ny.)  So a word asks for the real part of S (ny even) or the imaginary part (ny odd), with the
// weight  w = coef * (-1)^(ny >> 1).
//
// Host planner (pauli_plan): terms sorted by (x mask, observable) are cut greedily into PASSES.  A pass
// streams the state once through LDS tiles of 2^12 amplitudes: the 4 lowest bit positions (global accesses
// stay in runs of 16 contiguous amplitudes) and 8 further positions that hold the X/Y support of every
// term of the pass; diagonal terms (x = 0) join the first pass.  Up to 12 qubits one workgroup holds the
// whole state: one pass, whatever the terms.  A word whose own support does not fit a tile (more than 8
// positions above the lowest 4) is STREAMED: psi[k] and psi[k ^ x] as 16-byte pairs straight from global
// memory, one launch per distinct x mask that serves every term with that mask -- two reads.
//
// Tile kernel: a work item keeps its 16 amplitudes (and their |psi|^2) in registers, the tile is staged
// once, and after one barrier the terms of the pass are walked in (observable, x) order: partner chunk from
// LDS at (local index ^ local x), sign = parity(local index & local z) ^ parity(tile bits & outer z) -- the
// work item's share of the first parity and the whole second one are computed once per term, the share of
// the 16 register slots is wave-uniform.  The signed sum of a term is weighted in fp64 into the
// observable's accumulator; at each change of observable a wave adds its total into ITS slot of the
// partial table [state][observable][tile * 4 + wave] (zeroed per call; passes are ordered on the stream,
// every slot has one writer per pass; a streamed launch covers 2^12 contiguous amplitudes per workgroup
// and adds into the same slots).  k_pauli_final adds the slots of a column in fixed order in fp64:
// no atomics, the same bits from call to call.
//
// Applying a sum of words (qmle_apply_pauli_sum, the seed lambda = H psi of the adjoint sweep): with the sign
// taken at the row index as above,  (P psi)[i] = (-i)^ny (-1)^popc(i & z) psi[i ^ x].  Terms with equal (x, z)
// are merged on the host into unique WORDS, numbered in (x, z) order; k_pauli_coef adds, per sample and word, the
// products weight[b][obs] * coef * (-1)^(ny >> 1) of the word's terms in fp64 (a CSR over the terms).  What is
// left of the phase is 1 (ny even) or -i (ny odd).  The words go through the SAME planner (a word is a "term"
// whose column is its own number), so the tiles and the streamed masks are those of the measurement:
// k_pauli_apply_tile stages a tile of psi, keeps 16 complex output accumulators per work item and walks the
// pass's words; k_pauli_apply_stream forms, per distinct wide x mask, the signed sum d_x(i) of that mask's
// coefficients and adds d_x(i) psi[i ^ x].  The first launch of a call stores lambda, later ones add to it: one
// writer per element per launch, launches ordered on the stream -- no atomics, the same bits from call to call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <new>
#include <vector>

#include "qmle_sv.h"
#include "qmle_dev.h"
#include "qmle_host.h"

namespace {

constexpr int kPauliTileBits = 12;   // amplitudes of a tile: 32 KiB complex64, 64 KiB complex128
constexpr int kPauliLowBits = 4;     // lowest positions, in every tile
constexpr int kPauliWaves = 4;       // waves of a tile workgroup = partial slots per tile
constexpr int kPauliDensTerms = 64;  // terms per launch of the density kernel (passed by value)
constexpr int kPauliMaxTerms = 65536, kPauliMaxObs = 4096, kPauliMaxQubits = 30;

template <class R> struct Cx;
template <> struct Cx<float> { typedef float2 type; typedef float4 chunk; };
template <> struct Cx<double> { typedef double2 type; typedef double2 chunk; };

struct PauliTile {   // geometry of a pass
  int32_t n, T;
  uint8_t pos[kPauliTileBits];  // state-index position of local bit k, ascending
};
struct PauliTermDev {
  uint32_t xl, zl;   // x / z on the tile's positions, compacted to local bits
  uint32_t zo;       // z on the other positions (state-index positions)
  int32_t obs;
  double w;          // coef * (-1)^(ny >> 1)
  int32_t im;        // ny odd: the imaginary part of S
  int32_t pad;
};
struct PauliDens {
  uint32_t x[kPauliDensTerms], z[kPauliDensTerms];
  double w[kPauliDensTerms];   // coef and the sign of the part taken
  int16_t obs[kPauliDensTerms];
  int8_t im[kPauliDensTerms];
  int32_t count, obs_lo;       // the launch's observables are obs_lo .. obs_lo + gridDim.y - 1
};

__device__ __forceinline__ float re_cc(float2 a, float2 b) { return fmaf(a.y, b.y, a.x * b.x); }
__device__ __forceinline__ float im_cc(float2 a, float2 b) { return fmaf(-a.y, b.x, a.x * b.y); }
__device__ __forceinline__ double re_cc(double2 a, double2 b) { return fma(a.y, b.y, a.x * b.x); }
__device__ __forceinline__ double im_cc(double2 a, double2 b) { return fma(-a.y, b.x, a.x * b.y); }

// the amplitudes of a 16-byte chunk, and the chunk with its two complex64 amplitudes exchanged
__device__ __forceinline__ void unpack(float4 c, float2 (&a)[2]) {
  a[0] = make_float2(c.x, c.y);
  a[1] = make_float2(c.z, c.w);
}
__device__ __forceinline__ void unpack(double2 c, double2 (&a)[1]) { a[0] = c; }
__device__ __forceinline__ float4 swap_halves(float4 c) { return make_float4(c.z, c.w, c.x, c.y); }
__device__ __forceinline__ double2 swap_halves(double2 c) { return c; }

// One pass.  grid (tiles, states); 256 work items x 16 amplitudes.  Local index of a work item's amplitude:
// chunk cl = t | (ch << 8) of A = 16 / sizeof(amplitude) amplitudes, l = cl * A + e.  LDS: the tile alone.
template <class R>
__global__ void __launch_bounds__(256)
k_pauli_tile(const typename Cx<R>::chunk *__restrict__ states, PauliTile g,
             const PauliTermDev *__restrict__ terms, int n_terms, int n_obs, int n_rows,
             double *__restrict__ partial) {
  typedef typename Cx<R>::type C;
  typedef typename Cx<R>::chunk Chunk;
  constexpr int A = (int)(sizeof(Chunk) / sizeof(C)), LB = A == 2 ? 1 : 0, NCH = 16 / A;
  extern __shared__ __attribute__((aligned(16))) char pauli_lds[];
  Chunk *tile = reinterpret_cast<Chunk *>(pauli_lds);
  const uint32_t t = threadIdx.x, b = blockIdx.y;
  const uint32_t n_chunks = (1u << g.T) >> LB;

  // tile id -> its bits on the positions outside the tile
  uint32_t tile_mask = 0, base = 0;
  for (int k = 0; k < g.T; ++k) tile_mask |= 1u << g.pos[k];
  for (int p = 0, q = 0; p < g.n; ++p)
    if (!((tile_mask >> p) & 1u)) base |= ((blockIdx.x >> q++) & 1u) << p;
  // this work item's local bits LB .. LB+7 on their state-index positions (local bit 0 is position 0)
  uint32_t mine = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (LB + k < g.T) mine |= ((t >> k) & 1u) << g.pos[LB + k];

  const Chunk *st = states + (((size_t)b << g.n) >> LB);
  C a[16];
  R p[16];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const uint32_t cl = t | ((uint32_t)ch << 8);
    uint32_t idx = base | mine;
#pragma unroll
    for (int k = 0; k < 4 - LB; ++k)
      if (LB + 8 + k < g.T) idx |= (((uint32_t)ch >> k) & 1u) << g.pos[LB + 8 + k];
    Chunk c = {};
    if (cl < n_chunks) {
      c = st[idx >> LB];
      tile[cl] = c;
    }
    C e[A];
    unpack(c, e);
#pragma unroll
    for (int j = 0; j < A; ++j) {
      a[ch * A + j] = e[j];
      p[ch * A + j] = e[j].x * e[j].x + e[j].y * e[j].y;
    }
  }
  __syncthreads();

  const auto *tc = as_constant(terms);
  const int lane = t & (kWave - 1), wave = t / kWave;
  double *row = partial + (size_t)b * n_obs * n_rows + (size_t)blockIdx.x * kPauliWaves + wave;
  double acc = 0.0;
  int cur = tc[0].obs;
  for (int k = 0; k < n_terms; ++k) {
    const uint32_t xl = tc[k].xl, zl = tc[k].zl;
    const int obs = tc[k].obs;
    if (obs != cur) {
      const double tot = wave_sum_d(acc);
      if (lane == 0) row[(size_t)cur * n_rows] += tot;
      acc = 0.0;
      cur = obs;
    }
    const R outer = (__popc(base & tc[k].zo) & 1) ? (R)-1 : (R)1;
    R s = 0;
    if (xl == 0) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const uint32_t lu = (((uint32_t)(u / A) << 8) << LB) | (uint32_t)(u % A);
        s = fma(p[u], (__popc(lu & zl) & 1) ? -outer : outer, s);
      }
    } else {
      // a work item beyond a small tile (its amplitudes are zeros) reads some chunk of the tile
      const uint32_t pt = (t ^ ((xl >> LB) & 255u)) & (n_chunks - 1u);
      const bool swap = LB && (xl & 1u);
      const bool im = tc[k].im != 0;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const uint32_t pc = (((uint32_t)ch << 8) ^ ((xl >> LB) & ~255u)) & (n_chunks - 1u);
        Chunk q = tile[pt | pc];
        if (swap) q = swap_halves(q);
        C e[A];
        unpack(q, e);
#pragma unroll
        for (int j = 0; j < A; ++j) {
          const uint32_t lu = (((uint32_t)ch << 8) << LB) | (uint32_t)j;
          const R v = im ? im_cc(a[ch * A + j], e[j]) : re_cc(a[ch * A + j], e[j]);
          s = fma(v, (__popc(lu & zl) & 1) ? -outer : outer, s);
        }
      }
    }
    if (__popc((t << LB) & zl) & 1) s = -s;
    acc = fma(tc[k].w, (double)s, acc);
  }
  const double tot = wave_sum_d(acc);
  if (lane == 0) row[(size_t)cur * n_rows] += tot;
}

// Streamed terms of one x mask (n >= 13): a workgroup covers 2^12 contiguous amplitudes, a work item keeps
// Re and Im of conj(psi_i) psi_{i ^ x} of its 16 amplitudes -- each (own, partner) pair is loaded once per
// mask -- and walks the mask's terms (observable order) like the tile kernel: local z = the 12 low
// positions, outer z = the rest, the same partial slots [state][observable][workgroup * 4 + wave].
template <class R>
__global__ void __launch_bounds__(256)
k_pauli_stream(const typename Cx<R>::chunk *__restrict__ states, int n, uint32_t x,
               const PauliTermDev *__restrict__ terms, int n_terms, int n_obs, int n_rows,
               double *__restrict__ partial) {
  typedef typename Cx<R>::type C;
  typedef typename Cx<R>::chunk Chunk;
  constexpr int A = (int)(sizeof(Chunk) / sizeof(C)), LB = A == 2 ? 1 : 0, NCH = 16 / A;
  const uint32_t t = threadIdx.x, b = blockIdx.y;
  const uint32_t base = blockIdx.x << kPauliTileBits;
  const Chunk *st = states + (((size_t)b << n) >> LB);
  const uint32_t xc = x >> LB;
  const bool swap = LB && (x & 1u);
  R re[16], im[16];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const uint32_t c = (base >> LB) | ((uint32_t)ch << 8) | t;
    Chunk q = st[c ^ xc];
    if (swap) q = swap_halves(q);
    C own[A], par[A];
    unpack(st[c], own);
    unpack(q, par);
#pragma unroll
    for (int j = 0; j < A; ++j) {
      re[ch * A + j] = re_cc(own[j], par[j]);
      im[ch * A + j] = im_cc(own[j], par[j]);
    }
  }
  const auto *tc = as_constant(terms);
  const int lane = t & (kWave - 1), wave = t / kWave;
  double *row = partial + (size_t)b * n_obs * n_rows + (size_t)blockIdx.x * kPauliWaves + wave;
  double acc = 0.0;
  int cur = tc[0].obs;
  for (int k = 0; k < n_terms; ++k) {
    const uint32_t zl = tc[k].zl;
    const int obs = tc[k].obs;
    if (obs != cur) {
      const double tot = wave_sum_d(acc);
      if (lane == 0) row[(size_t)cur * n_rows] += tot;
      acc = 0.0;
      cur = obs;
    }
    const R outer = (__popc(base & tc[k].zo) & 1) ? (R)-1 : (R)1;
    const bool want_im = tc[k].im != 0;
    R s = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const uint32_t lu = (((uint32_t)(u / A) << 8) << LB) | (uint32_t)(u % A);
      s = fma(want_im ? im[u] : re[u], (__popc(lu & zl) & 1) ? -outer : outer, s);
    }
    if (__popc((t << LB) & zl) & 1) s = -s;
    acc = fma(tc[k].w, (double)s, acc);
  }
  const double tot = wave_sum_d(acc);
  if (lane == 0) row[(size_t)cur * n_rows] += tot;
}

// out[b][o] = the slots of column o in slot order.  grid (states, observables)
template <class R>
__global__ void __launch_bounds__(256)
k_pauli_final(const double *__restrict__ part, int n_rows, int n_obs, R *__restrict__ out) {
  __shared__ double red[16];
  const size_t col = (size_t)blockIdx.x * n_obs + blockIdx.y;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_rows; i += blockDim.x) acc += part[col * n_rows + i];
  const double tot = block_sum_d(acc, red);
  if (threadIdx.x == 0) out[col] = (R)tot;
}

// ---- lambda = (sum of weighted words) psi ----
// coef[b][w] = sum over the terms e of word w of weights[b][obs_e] * c_e, in fp64 and in term order; grid
// (words / 256, states).  c_e carries the term's coefficient and the sign (-1)^(ny >> 1) of its word.
template <class R>
__global__ void __launch_bounds__(256)
k_pauli_coef(const R *__restrict__ weights, int n_obs, const int32_t *__restrict__ ptr,
             const int32_t *__restrict__ obs, const double *__restrict__ c, int n_words, R *__restrict__ coef) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (w >= n_words) return;
  const R *row = weights + (size_t)b * n_obs;
  double acc = 0.0;
  for (int e = ptr[w]; e < ptr[w + 1]; ++e) acc = fma((double)row[obs[e]], c[e], acc);
  coef[(size_t)b * n_words + w] = (R)acc;
}

// acc += s * ph * v,  ph = -i (ny odd) or 1
template <class C, class R>
__device__ __forceinline__ void add_word(C &acc, R s, bool im, C v) {
  if (im) {
    acc.x = fma(s, v.y, acc.x);
    acc.y = fma(-s, v.x, acc.y);
  } else {
    acc.x = fma(s, v.x, acc.x);
    acc.y = fma(s, v.y, acc.y);
  }
}
__device__ __forceinline__ float4 pack(const float2 (&a)[2]) { return make_float4(a[0].x, a[0].y, a[1].x, a[1].y); }
__device__ __forceinline__ double2 pack(const double2 (&a)[1]) { return a[0]; }

// One pass: the geometry, the staging and the index arithmetic of k_pauli_tile.  `words` are the pass's words
// (PauliTermDev::obs = the word's column of coef [states][n_coef]; w is not read, the sign it holds is in the
// coefficient).  LDS: the tile of psi alone.  first != 0: out is stored, else added to.
template <class R>
__global__ void __launch_bounds__(256)
k_pauli_apply_tile(const typename Cx<R>::chunk *__restrict__ states, typename Cx<R>::chunk *__restrict__ out,
                   PauliTile g, const PauliTermDev *__restrict__ words, int n_words,
                   const R *__restrict__ coef, int n_coef, int first) {
  typedef typename Cx<R>::type C;
  typedef typename Cx<R>::chunk Chunk;
  constexpr int A = (int)(sizeof(Chunk) / sizeof(C)), LB = A == 2 ? 1 : 0, NCH = 16 / A;
  extern __shared__ __attribute__((aligned(16))) char pauli_lds[];
  Chunk *tile = reinterpret_cast<Chunk *>(pauli_lds);
  const uint32_t t = threadIdx.x, b = blockIdx.y;
  const uint32_t n_chunks = (1u << g.T) >> LB;

  uint32_t tile_mask = 0, base = 0;
  for (int k = 0; k < g.T; ++k) tile_mask |= 1u << g.pos[k];
  for (int p = 0, q = 0; p < g.n; ++p)
    if (!((tile_mask >> p) & 1u)) base |= ((blockIdx.x >> q++) & 1u) << p;
  uint32_t mine = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (LB + k < g.T) mine |= ((t >> k) & 1u) << g.pos[LB + k];

  const size_t state_off = ((size_t)b << g.n) >> LB;
  uint32_t gidx[NCH];  // chunk index of this work item's chunk ch in its state
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const uint32_t cl = t | ((uint32_t)ch << 8);
    uint32_t idx = base | mine;
#pragma unroll
    for (int k = 0; k < 4 - LB; ++k)
      if (LB + 8 + k < g.T) idx |= (((uint32_t)ch >> k) & 1u) << g.pos[LB + 8 + k];
    gidx[ch] = idx >> LB;
    if (cl < n_chunks) tile[cl] = states[state_off + gidx[ch]];
  }
  __syncthreads();

  const auto *tc = as_constant(words);
  const auto *cf = as_constant(coef + (size_t)b * n_coef);
  C acc[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) acc[u].x = acc[u].y = (R)0;
  for (int k = 0; k < n_words; ++k) {
    const uint32_t xl = tc[k].xl, zl = tc[k].zl;
    R s = cf[tc[k].obs];
    if (s == (R)0) continue;  // (a word whose terms cancel, a sample whose weights leave it out)
    if (__popc(base & tc[k].zo) & 1) s = -s;
    const bool im = tc[k].im != 0;
    if (__popc((t << LB) & zl) & 1) s = -s;
    // a work item beyond a small tile (it stores nothing) reads some chunk of the tile
    const uint32_t pt = (t ^ ((xl >> LB) & 255u)) & (n_chunks - 1u);
    const bool swap = LB && (xl & 1u);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const uint32_t pc = (((uint32_t)ch << 8) ^ ((xl >> LB) & ~255u)) & (n_chunks - 1u);
      Chunk q = tile[pt | pc];
      if (swap) q = swap_halves(q);
      C e[A];
      unpack(q, e);
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const uint32_t lu = (((uint32_t)ch << 8) << LB) | (uint32_t)j;
        add_word(acc[ch * A + j], (__popc(lu & zl) & 1) ? -s : s, im, e[j]);
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const uint32_t cl = t | ((uint32_t)ch << 8);
    if (cl >= n_chunks) continue;
    C e[A];
#pragma unroll
    for (int j = 0; j < A; ++j) e[j] = acc[ch * A + j];
    if (!first) {
      C old[A];
      unpack(out[state_off + gidx[ch]], old);
#pragma unroll
      for (int j = 0; j < A; ++j) {
        e[j].x += old[j].x;
        e[j].y += old[j].y;
      }
    }
    out[state_off + gidx[ch]] = pack(e);
  }
}

// The words of one x mask too wide for a tile (n >= 13), the shape of k_pauli_stream: a workgroup covers 2^12
// contiguous amplitudes, a work item first adds the mask's coefficients into d_x(i) for its 16 amplitudes
// (local z = the 12 low positions, outer z = the rest), then out[i] (+)= d_x(i) psi[i ^ x], one 16-byte
// partner chunk at a time.
template <class R>
__global__ void __launch_bounds__(256)
k_pauli_apply_stream(const typename Cx<R>::chunk *__restrict__ states, typename Cx<R>::chunk *__restrict__ out,
                     int n, uint32_t x, const PauliTermDev *__restrict__ words, int n_words,
                     const R *__restrict__ coef, int n_coef, int first) {
  typedef typename Cx<R>::type C;
  typedef typename Cx<R>::chunk Chunk;
  constexpr int A = (int)(sizeof(Chunk) / sizeof(C)), LB = A == 2 ? 1 : 0, NCH = 16 / A;
  const uint32_t t = threadIdx.x, b = blockIdx.y;
  const uint32_t base = blockIdx.x << kPauliTileBits;
  const size_t state_off = ((size_t)b << n) >> LB;
  const auto *tc = as_constant(words);
  const auto *cf = as_constant(coef + (size_t)b * n_coef);
  C d[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) d[u].x = d[u].y = (R)0;
  for (int k = 0; k < n_words; ++k) {
    const uint32_t zl = tc[k].zl;
    R s = cf[tc[k].obs];
    if (__popc(base & tc[k].zo) & 1) s = -s;
    if (__popc((t << LB) & zl) & 1) s = -s;
    const bool im = tc[k].im != 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const uint32_t lu = (((uint32_t)(u / A) << 8) << LB) | (uint32_t)(u % A);
      const R v = (__popc(lu & zl) & 1) ? -s : s;
      if (im) d[u].y -= v; else d[u].x += v;
    }
  }
  const uint32_t xc = x >> LB;
  const bool swap = LB && (x & 1u);
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const uint32_t c = (base >> LB) | ((uint32_t)ch << 8) | t;
    Chunk q = states[state_off + (c ^ xc)];
    if (swap) q = swap_halves(q);
    C par[A], e[A];
    unpack(q, par);
    if (first) {
#pragma unroll
      for (int j = 0; j < A; ++j) e[j].x = e[j].y = (R)0;
    } else {
      unpack(out[state_off + c], e);
    }
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const C dd = d[ch * A + j];
      e[j].x = fma(dd.x, par[j].x, fma(-dd.y, par[j].y, e[j].x));
      e[j].y = fma(dd.x, par[j].y, fma(dd.y, par[j].x, e[j].y));
    }
    out[state_off + c] = pack(e);
  }
}

// Tr(P rho) = sum_j i^ny (-1)^popc((j ^ x) & z) rho[j ^ x][j] for the terms of one launch; grid (states,
// observables of the launch).  Terms arrive sorted by observable, 64 per launch; d_out is zeroed by the call and a
// launch adds its fp64 sum (an observable of more than 64 words is therefore added in float32 across launches,
// ordered on the stream).
__global__ void __launch_bounds__(256)
k_density_pauli(const float2 *__restrict__ rho, int n, PauliDens pd, int n_obs, float *__restrict__ out) {
  __shared__ double red[16];
  const int b = blockIdx.x, o = pd.obs_lo + blockIdx.y;
  const uint32_t D = 1u << n;
  const float2 *r = rho + ((size_t)b << (2 * n));
  double acc = 0.0;
  for (int k = 0; k < pd.count; ++k) {
    if (pd.obs[k] != o) continue;
    double s = 0.0;
    for (uint32_t j = threadIdx.x; j < D; j += blockDim.x) {
      const uint32_t i = j ^ pd.x[k];
      const float2 v = r[(size_t)i * D + j];
      const float part = pd.im[k] ? v.y : v.x;
      s += (__popc(i & pd.z[k]) & 1) ? -(double)part : (double)part;
    }
    acc = fma(pd.w[k], s, acc);
  }
  const double tot = block_sum_d(acc, red);
  if (threadIdx.x == 0) {
    out[(size_t)b * n_obs + o] += (float)tot;
  }
}

// ---- host planner ----
struct PTerm {
  uint32_t x, z;  // bit positions
  int32_t obs, im;
  double w;
};
struct PPass {
  PauliTile geo;
  std::vector<PauliTermDev> terms;
};
struct PStream {  // every term of one x mask too wide for a tile
  uint32_t x;
  std::vector<PauliTermDev> terms;
};
struct PPlan {
  std::vector<PPass> passes;
  std::vector<PStream> streams;
  int reads() const { return (int)passes.size() + 2 * (int)streams.size(); }
};
int tile_rows(int n) { return (n > kPauliTileBits ? 1 << (n - kPauliTileBits) : 1) * kPauliWaves; }

// status of the arguments every entry point shares
int check_terms(int n_qubits, const qmle_pauli_term *terms, int n_terms, int n_obs, int max_qubits) {
  if (!terms || n_terms < 1 || n_terms > kPauliMaxTerms || n_obs < 1 || n_obs > kPauliMaxObs ||
      n_qubits < 1 || n_qubits > max_qubits)
    return QMLE_ERR_INVALID_ARG;
  for (int k = 0; k < n_terms; ++k)
    if (terms[k].obs < 0 || terms[k].obs >= n_obs) return QMLE_ERR_INVALID_ARG;
  for (int k = 0; k < n_terms; ++k)
    if ((terms[k].x_wires | terms[k].z_wires) >> n_qubits) return QMLE_ERR_WIRE_RANGE;
  return QMLE_OK;
}

std::vector<PTerm> to_positions(int n, const qmle_pauli_term *terms, int n_terms) {
  std::vector<PTerm> out((size_t)n_terms);
  for (int k = 0; k < n_terms; ++k) {
    PTerm &t = out[k];
    t.x = wires_to_pos(terms[k].x_wires, n);
    t.z = wires_to_pos(terms[k].z_wires, n);
    const int ny = __builtin_popcount(t.x & t.z);
    t.obs = terms[k].obs;
    t.im = ny & 1;
    t.w = (ny & 2) ? -terms[k].coef : terms[k].coef;
  }
  return out;
}

uint32_t compact(uint32_t mask, const PauliTile &g) {
  uint32_t m = 0;
  for (int k = 0; k < g.T; ++k) m |= ((mask >> g.pos[k]) & 1u) << k;
  return m;
}

// `high`: the positions above the lowest 4 that the pass's terms flip (at most 8); padded from below
PPass make_pass(int n, uint32_t high, const std::vector<PTerm> &terms) {
  PPass ps;
  ps.geo.n = n;
  ps.geo.T = n < kPauliTileBits ? n : kPauliTileBits;
  uint32_t mask = n <= kPauliTileBits ? (1u << n) - 1u : (high | ((1u << kPauliLowBits) - 1u));
  for (int p = kPauliLowBits; __builtin_popcount(mask) < ps.geo.T; ++p) mask |= 1u << p;
  for (int p = 0, k = 0; p < n; ++p)
    if ((mask >> p) & 1u) ps.geo.pos[k++] = (uint8_t)p;
  for (int k = ps.geo.T; k < kPauliTileBits; ++k) ps.geo.pos[k] = 0;
  std::vector<PTerm> sorted(terms);
  std::stable_sort(sorted.begin(), sorted.end(), [](const PTerm &a, const PTerm &b) {
    return a.obs != b.obs ? a.obs < b.obs : a.x < b.x;
  });
  for (const PTerm &t : sorted)
    ps.terms.push_back({compact(t.x, ps.geo), compact(t.z, ps.geo), t.z & ~mask, t.obs, t.w, t.im, 0});
  return ps;
}

PPlan pauli_plan(int n, const qmle_pauli_term *terms, int n_terms) {
  std::vector<PTerm> all = to_positions(n, terms, n_terms);
  std::stable_sort(all.begin(), all.end(), [](const PTerm &a, const PTerm &b) {
    return a.x != b.x ? a.x < b.x : a.obs < b.obs;
  });
  PPlan plan;
  if (n <= kPauliTileBits) {
    plan.passes.push_back(make_pass(n, 0u, all));
    return plan;
  }
  const uint32_t low = (1u << kPauliLowBits) - 1u;
  const int room = kPauliTileBits - kPauliLowBits;
  std::vector<std::pair<uint32_t, std::vector<PTerm>>> cuts;  // (high positions, terms) per pass
  std::vector<PTerm> diagonal;
  for (const PTerm &t : all) {
    const uint32_t hi = t.x & ~low;
    if (t.x == 0) {
      diagonal.push_back(t);
    } else if (__builtin_popcount(hi) > room) {
      // (sorted by x mask, then observable: a mask's terms arrive together, in the order the kernel flushes)
      if (plan.streams.empty() || plan.streams.back().x != t.x) plan.streams.push_back({t.x, {}});
      const uint32_t local = (1u << kPauliTileBits) - 1u;
      plan.streams.back().terms.push_back({0u, t.z & local, t.z & ~local, t.obs, t.w, t.im, 0});
    } else {
      if (cuts.empty() || __builtin_popcount(cuts.back().first | hi) > room) cuts.push_back({0u, {}});
      cuts.back().first |= hi;
      cuts.back().second.push_back(t);
    }
  }
  if (!diagonal.empty()) {
    if (cuts.empty()) cuts.push_back({0u, {}});
    cuts.front().second.insert(cuts.front().second.end(), diagonal.begin(), diagonal.end());
  }
  for (const auto &c : cuts) plan.passes.push_back(make_pass(n, c.first, c.second));
  return plan;
}

struct PauliLayout {
  int rows, chunk;   // partial slots per column, states per launch
  size_t table_bytes, part_bytes, total;
};
PauliLayout pauli_layout(int n, int batch, int n_terms, int n_obs) {
  PauliLayout L;
  L.rows = tile_rows(n);
  L.chunk = batch < kMaxGridY ? batch : kMaxGridY;
  L.table_bytes = align_up((size_t)n_terms * sizeof(PauliTermDev), 256);
  L.part_bytes = (size_t)L.chunk * n_obs * L.rows * sizeof(double);
  L.total = L.table_bytes + L.part_bytes + 256;
  return L;
}

template <class R>
int run_pauli(const void *d_states, int n, int batch, const qmle_pauli_term *terms, int n_terms, int n_obs,
              R *d_out, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  typedef typename Cx<R>::type C;
  typedef typename Cx<R>::chunk Chunk;
  constexpr bool f64 = sizeof(R) == 8;
  if (!d_states || !d_out || !d_ws || batch < 1) return QMLE_ERR_INVALID_ARG;
  const int rc = check_terms(n, terms, n_terms, n_obs, kPauliMaxQubits);
  if (rc != QMLE_OK) return rc;
  const PauliLayout L = pauli_layout(n, batch, n_terms, n_obs);
  if (ws_bytes < L.total) return QMLE_ERR_INVALID_ARG;
  char *ws = (char *)d_ws;
  if (!align_workspace(ws, ws_bytes)) return QMLE_ERR_INVALID_ARG;

  const PPlan plan = pauli_plan(n, terms, n_terms);
  std::vector<PauliTermDev> table;
  for (const PPass &ps : plan.passes) table.insert(table.end(), ps.terms.begin(), ps.terms.end());
  for (const PStream &ps : plan.streams) table.insert(table.end(), ps.terms.begin(), ps.terms.end());
  PauliTermDev *d_terms = (PauliTermDev *)ws;
  if (!table.empty())
    HIPCHK(hipMemcpyAsync(d_terms, table.data(), table.size() * sizeof(PauliTermDev), hipMemcpyHostToDevice, stream));
  double *tile_part = (double *)(ws + L.table_bytes);
  const size_t lds = sizeof(C) << (n < kPauliTileBits ? n : kPauliTileBits);
  if (f64) {
    if (FirstUse once{0}; once.first) {
      HIPCHK(hipFuncSetAttribute((const void *)k_pauli_tile<R>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(sizeof(C) << kPauliTileBits)));
      once.done();
    }
  }
  const size_t amps = (size_t)1 << n;
  for (int b0 = 0; b0 < batch; b0 += L.chunk) {
    const int bc = batch - b0 < L.chunk ? batch - b0 : L.chunk;
    const Chunk *st = (const Chunk *)((const C *)d_states + (size_t)b0 * amps);
    HIPCHK(hipMemsetAsync(tile_part, 0, (size_t)bc * n_obs * L.rows * sizeof(double), stream));
    size_t off = 0;
    for (const PPass &ps : plan.passes) {
      hipLaunchKernelGGL(k_pauli_tile<R>, dim3(L.rows / kPauliWaves, bc), dim3(256), lds, stream, st, ps.geo,
                         d_terms + off, (int)ps.terms.size(), n_obs, L.rows, tile_part);
      off += ps.terms.size();
    }
    for (const PStream &ps : plan.streams) {
      hipLaunchKernelGGL(k_pauli_stream<R>, dim3(L.rows / kPauliWaves, bc), dim3(256), 0, stream, st, n, ps.x,
                         d_terms + off, (int)ps.terms.size(), n_obs, L.rows, tile_part);
      off += ps.terms.size();
    }
    hipLaunchKernelGGL(k_pauli_final<R>, dim3(bc, n_obs), dim3(L.rows >= 256 ? 256 : 64), 0, stream, tile_part,
                       L.rows, n_obs, d_out + (size_t)b0 * n_obs);
    HIPCHK(hipGetLastError());
  }
  return QMLE_OK;
}

// ---- lambda = (sum of weighted words) psi: host ----
struct SeedLayout {
  int chunk;  // states per launch
  size_t table, ptr, obs, c, coef, total;
};
// (every table is sized by the term count, which bounds the word count: the query needs no plan)
SeedLayout seed_layout(int batch, int n_terms, bool f64) {
  SeedLayout L;
  L.chunk = batch < kMaxGridY ? batch : kMaxGridY;
  L.table = 0;
  L.ptr = L.table + align_up((size_t)n_terms * sizeof(PauliTermDev), 256);
  L.obs = L.ptr + align_up(((size_t)n_terms + 1) * sizeof(int32_t), 256);
  L.c = L.obs + align_up((size_t)n_terms * sizeof(int32_t), 256);
  L.coef = L.c + align_up((size_t)n_terms * sizeof(double), 256);
  L.total = L.coef + align_up((size_t)L.chunk * n_terms * (f64 ? 8 : 4), 256) + 256;
  return L;
}

// unique words in (x, z) order of their position masks, as planner input (column = the word's number, weight 1),
// and the CSR of their terms
struct SeedWords {
  std::vector<qmle_pauli_term> words;
  std::vector<int32_t> ptr, obs;
  std::vector<double> c;
};
SeedWords seed_words(int n, const qmle_pauli_term *terms, int n_terms) {
  const std::vector<PTerm> pos = to_positions(n, terms, n_terms);
  std::vector<int> order((size_t)n_terms);
  for (int k = 0; k < n_terms; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return pos[a].x != pos[b].x ? pos[a].x < pos[b].x : pos[a].z < pos[b].z;
  });
  SeedWords sw;
  for (int k : order) {
    if (sw.words.empty() || sw.words.back().x_wires != terms[k].x_wires || sw.words.back().z_wires != terms[k].z_wires) {
      sw.words.push_back({terms[k].x_wires, terms[k].z_wires, (int32_t)sw.words.size(), 1.0});
      sw.ptr.push_back((int32_t)sw.obs.size());
    }
    sw.obs.push_back(terms[k].obs);
    sw.c.push_back(pos[k].w);  // coef * (-1)^(ny >> 1)
  }
  sw.ptr.push_back((int32_t)sw.obs.size());
  return sw;
}
PPlan seed_plan(int n, const SeedWords &sw) { return pauli_plan(n, sw.words.data(), (int)sw.words.size()); }

}  // namespace

namespace qmle {

struct PauliSeed {
  int n, n_words, n_obs;
  bool f64;
  SeedLayout L;
  char *ws;
  PPlan plan;                       // empty for the flat table of the whole-sweep-in-LDS kernel
  std::vector<size_t> pass_off;     // first table entry of every pass, then of every streamed mask
};

int pauli_seed_check(int n_qubits, const qmle_pauli_term *terms, int n_terms, int n_obs) {
  return check_terms(n_qubits, terms, n_terms, n_obs, kPauliMaxQubits);
}
size_t pauli_seed_ws_bytes(int batch, int n_terms, bool f64) { return seed_layout(batch, n_terms, f64).total; }

int pauli_seed_begin(PauliSeed **out, int n, int max_batch, const qmle_pauli_term *terms, int n_terms, int n_obs,
                     bool f64, bool flat, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  *out = nullptr;
  char *ws = (char *)d_ws;
  const SeedLayout L = seed_layout(max_batch, n_terms, f64);
  if (!align_workspace(ws, ws_bytes) || ws_bytes < L.total - 256) return QMLE_ERR_INVALID_ARG;
  const SeedWords sw = seed_words(n, terms, n_terms);
  PauliSeed *sd = new (std::nothrow) PauliSeed{n, (int)sw.words.size(), n_obs, f64, L, ws, {}, {}};
  if (!sd) return QMLE_ERR_INTERNAL;
  std::unique_ptr<PauliSeed> hold(sd);
  if (flat) {
    std::vector<PauliWordDev> table;
    for (const qmle_pauli_term &w : sw.words) {
      const uint32_t x = wires_to_pos(w.x_wires, n), z = wires_to_pos(w.z_wires, n);
      table.push_back({x, z, __builtin_popcount(x & z) & 1, 0});
    }
    HIPCHK(hipMemcpyAsync(ws + L.table, table.data(), table.size() * sizeof(PauliWordDev), hipMemcpyHostToDevice, stream));
  } else {
    sd->plan = seed_plan(n, sw);
    std::vector<PauliTermDev> table;
    for (const PPass &ps : sd->plan.passes) {
      sd->pass_off.push_back(table.size());
      table.insert(table.end(), ps.terms.begin(), ps.terms.end());
    }
    for (const PStream &ps : sd->plan.streams) {
      sd->pass_off.push_back(table.size());
      table.insert(table.end(), ps.terms.begin(), ps.terms.end());
    }
    HIPCHK(hipMemcpyAsync(ws + L.table, table.data(), table.size() * sizeof(PauliTermDev), hipMemcpyHostToDevice, stream));
    if (f64) {
      if (FirstUse once{1}; once.first) {
        HIPCHK(hipFuncSetAttribute((const void *)k_pauli_apply_tile<double>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double2) << kPauliTileBits)));
        once.done();
      }
    }
  }
  HIPCHK(hipMemcpyAsync(ws + L.ptr, sw.ptr.data(), sw.ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(ws + L.obs, sw.obs.data(), sw.obs.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(ws + L.c, sw.c.data(), sw.c.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  *out = hold.release();
  return QMLE_OK;
}
void pauli_seed_end(PauliSeed *sd) { delete sd; }

template <class R>
static void seed_coef(const PauliSeed *sd, int batch, const void *d_weights, hipStream_t stream) {
  hipLaunchKernelGGL(k_pauli_coef<R>, dim3(grid_for((uint64_t)sd->n_words, 256), batch), dim3(256), 0, stream,
                     (const R *)d_weights, sd->n_obs, (const int32_t *)(sd->ws + sd->L.ptr),
                     (const int32_t *)(sd->ws + sd->L.obs), (const double *)(sd->ws + sd->L.c), sd->n_words,
                     (R *)(sd->ws + sd->L.coef));
}

int pauli_seed_flat(const PauliSeed *sd, int batch, const float *d_weights, hipStream_t stream,
                    const PauliWordDev **d_words, const float **d_coef, int *n_words) {
  if (batch > sd->L.chunk || sd->f64) return QMLE_ERR_INTERNAL;
  seed_coef<float>(sd, batch, d_weights, stream);
  HIPCHK(hipGetLastError());
  *d_words = (const PauliWordDev *)(sd->ws + sd->L.table);
  *d_coef = (const float *)(sd->ws + sd->L.coef);
  *n_words = sd->n_words;
  return QMLE_OK;
}

template <class R>
static int seed_apply(const PauliSeed *sd, const void *d_psi, void *d_lam, int batch, const void *d_weights,
                      hipStream_t stream) {
  typedef typename Cx<R>::type C;
  typedef typename Cx<R>::chunk Chunk;
  const int n = sd->n;
  const size_t lds = sizeof(C) << (n < kPauliTileBits ? n : kPauliTileBits);
  const unsigned tiles = n > kPauliTileBits ? 1u << (n - kPauliTileBits) : 1u;
  const PauliTermDev *d_table = (const PauliTermDev *)(sd->ws + sd->L.table);
  const R *d_coef = (const R *)(sd->ws + sd->L.coef);
  for (int b0 = 0; b0 < batch; b0 += sd->L.chunk) {
    const int bc = batch - b0 < sd->L.chunk ? batch - b0 : sd->L.chunk;
    const Chunk *st = (const Chunk *)((const C *)d_psi + ((size_t)b0 << n));
    Chunk *lam = (Chunk *)((C *)d_lam + ((size_t)b0 << n));
    seed_coef<R>(sd, bc, (const R *)d_weights + (size_t)b0 * sd->n_obs, stream);
    size_t k = 0;
    int first = 1;
    for (const PPass &ps : sd->plan.passes) {
      hipLaunchKernelGGL(k_pauli_apply_tile<R>, dim3(tiles, bc), dim3(256), lds, stream, st, lam, ps.geo,
                         d_table + sd->pass_off[k++], (int)ps.terms.size(), d_coef, sd->n_words, first);
      first = 0;
    }
    for (const PStream &ps : sd->plan.streams) {
      hipLaunchKernelGGL(k_pauli_apply_stream<R>, dim3(tiles, bc), dim3(256), 0, stream, st, lam, n, ps.x,
                         d_table + sd->pass_off[k++], (int)ps.terms.size(), d_coef, sd->n_words, first);
      first = 0;
    }
    HIPCHK(hipGetLastError());
  }
  return QMLE_OK;
}
int pauli_seed_apply(const PauliSeed *sd, const void *d_psi, void *d_lam, int batch, const void *d_weights,
                     hipStream_t stream) {
  if (sd->plan.passes.empty() && sd->plan.streams.empty()) return QMLE_ERR_INTERNAL;
  return sd->f64 ? seed_apply<double>(sd, d_psi, d_lam, batch, d_weights, stream)
                 : seed_apply<float>(sd, d_psi, d_lam, batch, d_weights, stream);
}

}  // namespace qmle

namespace {

int run_apply(const void *d_states, int n, int batch, const qmle_pauli_term *terms, int n_terms, int n_obs,
              const void *d_weights, void *d_out, void *d_ws, size_t ws_bytes, bool f64, hipStream_t stream) {
  if (!d_states || !d_out || !d_weights || !d_ws || batch < 1 || d_out == d_states) return QMLE_ERR_INVALID_ARG;
  int rc = check_terms(n, terms, n_terms, n_obs, kPauliMaxQubits);
  if (rc != QMLE_OK) return rc;
  if (ws_bytes < seed_layout(batch, n_terms, f64).total) return QMLE_ERR_INVALID_ARG;
  PauliSeed *sd = nullptr;
  rc = pauli_seed_begin(&sd, n, batch, terms, n_terms, n_obs, f64, false, d_ws, ws_bytes, stream);
  if (rc != QMLE_OK) return rc;
  rc = pauli_seed_apply(sd, d_states, d_out, batch, d_weights, stream);
  pauli_seed_end(sd);
  return rc;
}

}  // namespace

extern "C" {

size_t qmle_expval_pauli_workspace_bytes(int n_qubits, int batch, int n_terms, int n_obs) {
  if (n_qubits < 1 || n_qubits > kPauliMaxQubits || batch < 1 || n_terms < 1 || n_obs < 1) return 0;
  return pauli_layout(n_qubits, batch, n_terms, n_obs).total;
}
size_t qmle_expval_pauli_workspace_bytes_f64(int n_qubits, int batch, int n_terms, int n_obs) {
  if (n_qubits < 1 || n_qubits > kPauliMaxQubits || batch < 1 || n_terms < 1 || n_obs < 1) return 0;
  return pauli_layout(n_qubits, batch, n_terms, n_obs).total;
}

int qmle_expval_pauli(const void *d_states, int n_qubits, int batch, const qmle_pauli_term *terms,
                      int n_terms, int n_obs, float *d_out, void *d_ws, size_t ws_bytes, qmle_stream stream) {
  return run_pauli<float>(d_states, n_qubits, batch, terms, n_terms, n_obs, d_out, d_ws, ws_bytes,
                          (hipStream_t)stream);
}
int qmle_expval_pauli_f64(const void *d_states, int n_qubits, int batch, const qmle_pauli_term *terms,
                          int n_terms, int n_obs, double *d_out, void *d_ws, size_t ws_bytes,
                          qmle_stream stream) {
  return run_pauli<double>(d_states, n_qubits, batch, terms, n_terms, n_obs, d_out, d_ws, ws_bytes,
                           (hipStream_t)stream);
}

int qmle_expval_pauli_reads(int n_qubits, const qmle_pauli_term *terms, int n_terms, int f64) {
  (void)f64;  // both engines cut the same tiles
  const int rc = check_terms(n_qubits, terms, n_terms, kPauliMaxObs, kPauliMaxQubits);
  if (rc != QMLE_OK) return rc;
  return pauli_plan(n_qubits, terms, n_terms).reads();
}

size_t qmle_apply_pauli_sum_workspace_bytes(int n_qubits, int batch, int n_terms, int n_obs) {
  if (n_qubits < 1 || n_qubits > kPauliMaxQubits || batch < 1 || n_terms < 1 || n_obs < 1) return 0;
  return seed_layout(batch, n_terms, false).total;
}
size_t qmle_apply_pauli_sum_workspace_bytes_f64(int n_qubits, int batch, int n_terms, int n_obs) {
  if (n_qubits < 1 || n_qubits > kPauliMaxQubits || batch < 1 || n_terms < 1 || n_obs < 1) return 0;
  return seed_layout(batch, n_terms, true).total;
}
int qmle_apply_pauli_sum(const void *d_states, int n_qubits, int batch, const qmle_pauli_term *terms, int n_terms,
                         int n_obs, const float *d_weights, void *d_out, void *d_ws, size_t ws_bytes,
                         qmle_stream stream) {
  return run_apply(d_states, n_qubits, batch, terms, n_terms, n_obs, d_weights, d_out, d_ws, ws_bytes, false,
                   (hipStream_t)stream);
}
int qmle_apply_pauli_sum_f64(const void *d_states, int n_qubits, int batch, const qmle_pauli_term *terms,
                             int n_terms, int n_obs, const double *d_weights, void *d_out, void *d_ws,
                             size_t ws_bytes, qmle_stream stream) {
  return run_apply(d_states, n_qubits, batch, terms, n_terms, n_obs, d_weights, d_out, d_ws, ws_bytes, true,
                   (hipStream_t)stream);
}
int qmle_apply_pauli_sum_reads(int n_qubits, const qmle_pauli_term *terms, int n_terms, int f64) {
  (void)f64;  // both engines cut the same tiles
  const int rc = check_terms(n_qubits, terms, n_terms, kPauliMaxObs, kPauliMaxQubits);
  if (rc != QMLE_OK) return rc;
  return seed_plan(n_qubits, seed_words(n_qubits, terms, n_terms)).reads();
}

int qmle_density_expval_pauli(const void *d_rho, int n_qubits, int batch, const qmle_pauli_term *terms,
                              int n_terms, int n_obs, float *d_out, qmle_stream stream) {
  if (!d_rho || !d_out || batch < 1) return QMLE_ERR_INVALID_ARG;
  const int rc = check_terms(n_qubits, terms, n_terms, n_obs, QMLE_MAX_QUBITS / 2);
  if (rc != QMLE_OK) return rc;
  std::vector<PTerm> all = to_positions(n_qubits, terms, n_terms);
  for (int k = 0; k < n_terms; ++k) all[k].w = terms[k].coef;
  std::stable_sort(all.begin(), all.end(), [](const PTerm &a, const PTerm &b) { return a.obs < b.obs; });
  HIPCHK(hipMemsetAsync(d_out, 0, (size_t)batch * n_obs * sizeof(float), (hipStream_t)stream));
  for (int k0 = 0; k0 < n_terms; k0 += kPauliDensTerms) {
    PauliDens pd = {};
    pd.count = n_terms - k0 < kPauliDensTerms ? n_terms - k0 : kPauliDensTerms;
    pd.obs_lo = all[(size_t)k0].obs;
    const int obs_count = all[(size_t)k0 + pd.count - 1].obs - pd.obs_lo + 1;
    for (int k = 0; k < pd.count; ++k) {
      const PTerm &t = all[(size_t)k0 + k];
      const int ny = __builtin_popcount(t.x & t.z) & 3;
      pd.x[k] = t.x;
      pd.z[k] = t.z;
      pd.obs[k] = (int16_t)t.obs;
      pd.im[k] = (int8_t)(ny & 1);
      // Re(i^ny v): Re v, -Im v, -Re v, Im v
      pd.w[k] = (ny == 1 || ny == 2) ? -t.w : t.w;
    }
    for (int b0 = 0; b0 < batch; b0 += kMaxGridY) {
      const int bc = batch - b0 < kMaxGridY ? batch - b0 : kMaxGridY;
      hipLaunchKernelGGL(k_density_pauli, dim3(bc, obs_count), dim3(256), 0, (hipStream_t)stream,
                         (const float2 *)d_rho + ((size_t)b0 << (2 * n_qubits)), n_qubits, pd, n_obs,
                         d_out + (size_t)b0 * n_obs);
    }
  }
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

}  // extern "C"
