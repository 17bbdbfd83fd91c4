// libqmle_sv, adjoint differentiation in complex64.  adjoint_run checks a call, lays out its workspace and takes one
// of three routes: the whole sweep in LDS (n <= 13, adj_run_lds), or the forward run and the seed followed by the
// reverse plan's stages (adj_run_stages) -- fused tile passes over psi and lambda (n >= 14, tables from
// adj_fused_tables) or one streaming overlap per gate.  The kernels, checks, launch pairs and entry-point bodies that
// the complex128 sweep of qmle_f64.hip has too sit in qmle_adjoint_dev.h.
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
#include "qmle_adjoint_dev.h"
#include "qmle_density_dev.h"
#include "qmle_tile_dev.h"

namespace {

// ---- whole-circuit adjoint in LDS (n <= 13) ----------------------------------------------
// One workgroup per sample keeps psi AND lambda in LDS: forward circuit (fused gate groups),
// lambda = (sum_k w_k Z_k) psi -- or, <PAULI>, lambda = sum_words c[b][word] ph (-1)^popc(i & z) psi[i ^ x] from
// the flat word table and the coefficient rows of qmle_pauli.hip -- then for every gate of the reversed, daggered
// tape the generator overlap and the inverse gate on both vectors.  No HBM traffic beyond the angle
// tables and the gradient row; one launch instead of ~(2 gates + 2 angles) launches.
struct AdjTermDev {
  int32_t out_slot;
  uint32_t xmask, zmask, pmask;  // bit positions
  int32_t n_y;
  float coef;
  int32_t marks_off;             // offset in the reverse plan's const blob, or -1
  int32_t cot_off;               // offset, in floats, of the matrix cotangent this op reports in the sample's row, or -1
};
struct AdjLdsArgs {
  TileArgs fwd;                  // the forward plan's whole-state stage
  const LoweredOp *rev_ops;      // reverse tape, global bit positions, one gate each
  const AdjTermDev *terms;
  int n_rev;
  const float *rev_mats;
  uint32_t rev_mat_floats;
  const float *rev_angles;
  int rev_n_slots;
  const float *rev_consts;
  const float *weights;          // [B][n_obs]
  union {                        // the seed: Z-parity masks, or <PAULI> words and their coefficient rows
    ZMasks z;
    struct {
      const PauliWordDev *words;
      const float *coef;         // [B][n_words]
      int n_words;
    } pw;
  };
  int n_obs;
  float *grad;
  int n_grad_slots;
  float *cot;                    // [B][cot_stride] matrix cotangents (blocks of 8 or 32 floats), or nullptr
  int cot_stride;
};

// eight per-thread sums -> their workgroup totals, valid in thread 0; `red`: eight floats per wave
__device__ __forceinline__ void block_sum8(float (&m)[8], float *red) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave, nw = (blockDim.x + kWave - 1) / kWave;
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = wave_sum(m[k]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wv * 8 + k] = m[k];
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < nw; ++i) {
#pragma unroll
      for (int k = 0; k < 8; ++k) m[k] += red[i * 8 + k];
    }
  }
}

template <bool DENSE4, bool PAULI>
__global__ void k_adjoint_lds(const AdjLdsArgs a) {
  extern __shared__ float4 smem4[];
  const int T = a.fwd.T;
  float2 *psi = reinterpret_cast<float2 *>(smem4);
  float2 *lam = psi + (1u << T);
  float *red = reinterpret_cast<float *>(lam + (1u << T));
  OpSlot *slots = reinterpret_cast<OpSlot *>(red + 288);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int b = blockIdx.y;
  const uint32_t cnt = 1u << T;

  if (a.fwd.slots_in_lds) tile_stage_slots(a.fwd, slots, b);
  for (uint32_t e = tid; e < cnt; e += nt) psi[e] = make_float2(0.f, 0.f);
  __syncthreads();
  if (tid == 0) psi[sw(0)] = make_float2(1.f, 0.f);
  __syncthreads();
  tile_compute<DENSE4>(a.fwd, psi, slots, b);

  if constexpr (PAULI) {
    const float *cf = a.pw.coef + (size_t)b * a.pw.n_words;
    for (uint32_t i = tid; i < cnt; i += nt) {
      float2 acc = make_float2(0.f, 0.f);
      for (int k = 0; k < a.pw.n_words; ++k) {
        const PauliWordDev wd = a.pw.words[k];
        const float c = (__popc(i & wd.z) & 1) ? -cf[k] : cf[k];
        const float2 v = psi[sw(i ^ wd.x)];
        if (wd.im) {  // -i v
          acc.x = fmaf(c, v.y, acc.x);
          acc.y = fmaf(-c, v.x, acc.y);
        } else {
          acc.x = fmaf(c, v.x, acc.x);
          acc.y = fmaf(c, v.y, acc.y);
        }
      }
      lam[sw(i)] = acc;
    }
  } else {
    const float *w = a.weights + (size_t)b * a.n_obs;
    for (uint32_t i = tid; i < cnt; i += nt) {
      float d = 0.f;
      for (int o = 0; o < a.n_obs; ++o) d += (__popc(i & a.z.mask[o]) & 1) ? -w[o] : w[o];
      const float2 v = psi[sw(i)];
      lam[sw(i)] = make_float2(d * v.x, d * v.y);
    }
  }
  __syncthreads();

  const float *mrow = a.rev_mats + (size_t)b * a.rev_mat_floats;
  const float *ang = a.rev_angles + (size_t)b * a.rev_n_slots;
  for (int r = 0; r < a.n_rev; ++r) {
    const AdjTermDev t = a.terms[r];
    if (t.out_slot >= 0) {
      const float *marks = t.marks_off >= 0 ? a.rev_consts + t.marks_off : nullptr;
      float re = 0.f, im = 0.f;
      for (uint32_t i = tid; i < cnt; i += nt) {
        if ((i & t.pmask) != t.pmask) continue;
        const uint32_t j = i ^ t.xmask;
        const float2 l = lam[sw(i)], p = psi[sw(j)];
        const float sgn = marks ? marks[i] : ((__popc(j & t.zmask) & 1) ? -1.f : 1.f);
        re += sgn * (l.x * p.x + l.y * p.y);
        im += sgn * (l.x * p.y - l.y * p.x);
      }
      const float sr = block_sum(re, red);
      const float si = block_sum(im, red);
      if (tid == 0) a.grad[(size_t)b * a.n_grad_slots + t.out_slot] = t.coef * adj_phase(t.n_y, sr, si);
    }
    const LoweredOp o = a.rev_ops[r];
    if (t.cot_off >= 0 && o.kind == LK_1Q) {  // a one-wire matrix gate: all eight numbers from one read of both
      const uint32_t tb = 1u << o.t0;
      float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (uint32_t i = tid; i < (cnt >> 1); i += nt) {
        const uint32_t j0 = ins0(i, o.t0), j1 = j0 | tb;
        cot_accumulate(m, lam[sw(j0)], lam[sw(j1)], psi[sw(j0)], psi[sw(j1)]);
      }
      block_sum8(m, red);
      if (tid == 0) cot_finish<2>(m, mrow + o.mat_off, a.cot + (size_t)b * a.cot_stride + t.cot_off);
    } else if (t.cot_off >= 0) {  // a two-wire one (kinds checked on the host): one row of the 4x4 moment per pass
      const uint32_t b0 = 1u << o.t0, b1 = 1u << o.t1;
      const int plo = o.t0 < o.t1 ? o.t0 : o.t1, phi = o.t0 < o.t1 ? o.t1 : o.t0;
#pragma unroll 1
      for (int row = 0; row < 4; ++row) {
        const uint32_t la = ((row & 2) ? b0 : 0u) | ((row & 1) ? b1 : 0u);
        float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (uint32_t i = tid; i < (cnt >> 2); i += nt) {
          const uint32_t j = ins0(ins0(i, plo), phi);
          cot_row4(m, lam[sw(j | la)], psi[sw(j)], psi[sw(j | b1)], psi[sw(j | b0)], psi[sw(j | b0 | b1)]);
        }
        block_sum8(m, red);
        if (tid == 0) {  // (behind the per-wave sums: red holds 288 floats)
#pragma unroll
          for (int k = 0; k < 8; ++k) red[256 + row * 8 + k] = m[k];
        }
      }
      if (tid == 0) cot_finish<4>((const float *)(red + 256), mrow + o.mat_off, a.cot + (size_t)b * a.cot_stride + t.cot_off);
    }
    lds_apply(psi, T, o, mrow, a.rev_consts, ang);
    lds_apply(lam, T, o, mrow, a.rev_consts, ang);
    __syncthreads();
  }
}

// ---- fused adjoint tile pass (n >= 14) ----------------------------------------------------
// The backward sweep with the forward path's machinery: a pass stages the SAME tile of psi and
// of lambda in LDS, walks the register-tile groups of the reversed, daggered tape, and for every
// gate first takes the generator overlap Im <lambda| G |psi> on the 16 + 16 amplitudes a thread
// holds (G = X / Y / Z on the target, restricted to control = 1; P1 = |1><1| for CPhase), then
// applies the inverse gate to both.  One HBM round trip of the two states per ~20 gates instead
// of one per gate plus one per angle.
//   LoweredOp::slot (unused by 1-qubit ops) carries the stage-local index of the derivative
//   (-1: none), LoweredOp::pad the generator type.
enum AdjGen : int { AG_NONE = 0, AG_X = 1, AG_Y = 2, AG_Z = 3, AG_P1 = 4 };

// Im <y| G |x> on the 16 + 16 amplitudes of a register tile: G x by the gate appliers themselves
// (the generator as a 2x2 "gate"), so the only gate-shaped code in the sweep is reg_dispatch.
// With a control the applier leaves the control = 0 rows alone; those are taken out again with
// a second application whose matrix is zero ((Pbar + P G) x - Pbar x = P G x).
__device__ __forceinline__ Mat2 gen_matrix(int gtype) {
  Mat2 g;
  const float2 z = make_float2(0.f, 0.f), one = make_float2(1.f, 0.f);
  g.m00 = g.m01 = g.m10 = g.m11 = z;
  if (gtype == AG_X) { g.m01 = one; g.m10 = one; }
  else if (gtype == AG_Y) { g.m01 = make_float2(0.f, -1.f); g.m10 = make_float2(0.f, 1.f); }
  else if (gtype == AG_Z) { g.m00 = one; g.m11 = make_float2(-1.f, 0.f); }
  else { g.m11 = one; }  // AG_P1
  return g;
}
__device__ __forceinline__ float reg_im_dot(const float2 (&y)[16], const float2 (&t)[16]) {
  float im = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) im += y[c].x * t[c].y - y[c].y * t[c].x;
  return im;
}

struct AdjTileArgs {
  TileArgs t;               // stage of the reverse plan: groups, ops, matrices of sample b
  float2 *lam;              // [B][2^n]  (t.states = psi)
  const int32_t *term_idx;  // per dev_op of the stage: stage-local derivative index or -1
  const int32_t *gtype;     // per dev_op of the stage: AdjGen
  float *partial;           // [B][tiles][n_terms]
  int n_terms;
};

__global__ void __launch_bounds__(256) k_tile_adj(const AdjTileArgs A) {
  extern __shared__ float4 smem4[];
  const TileArgs &a = A.t;
  const int T = a.T, L = a.L;
  float2 *s0 = reinterpret_cast<float2 *>(smem4);
  float2 *s1 = s0 + (1u << T);
  uint32_t *lut = reinterpret_cast<uint32_t *>(s1 + (1u << T));
  const uint32_t lut_n = (1u << (T - L)) < 4u ? 4u : (1u << (T - L));
  OpSlot *slots = reinterpret_cast<OpSlot *>(lut + lut_n);
  float *ov = reinterpret_cast<float *>(slots + a.n_ops);  // [waves][n_terms]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & (kWave - 1), w = tid / kWave, nw = nt / kWave;
  const int b = blockIdx.y;
  const uint32_t tile = blockIdx.x;
  const size_t D = (size_t)1 << a.n;
  const uint64_t base = tile_base(a, tile);
  tile_build_lut(a, lut);
  {  // op descriptors + sample b's inverse-gate matrices + derivative bookkeeping -> LDS
    const float *mrow0 = a.mats + (size_t)b * a.mat_floats;
    for (int k = tid; k < a.n_ops; k += nt) {
      // LoweredOp as four words: {kind, flags, t0, t1}, {c0, c1, nc, pad}, mat_off, slot
      uint4 o = *reinterpret_cast<const uint4 *>(a.ops + a.op_begin + k);
      const float4 lo4 = *reinterpret_cast<const float4 *>(mrow0 + o.z);
      const float4 hi4 = *reinterpret_cast<const float4 *>(mrow0 + o.z + 4);
      o.y = (o.y & 0x00ffffffu) | ((uint32_t)A.gtype[k] << 24);  // pad  <- generator type
      o.w = (uint32_t)A.term_idx[k];                              // slot <- derivative index
      *reinterpret_cast<uint4 *>(&slots[k].op) = o;
      *reinterpret_cast<float4 *>(slots[k].m) = lo4;
      *reinterpret_cast<float4 *>(slots[k].m + 4) = hi4;
    }
    for (int k = tid; k < nw * A.n_terms; k += nt) ov[k] = 0.f;
  }
  __syncthreads();
  const uint32_t half = 1u << (T - 1), lowmask = (1u << L) - 1u;
  float2 *st0 = a.states + (size_t)b * D, *st1 = A.lam + (size_t)b * D;
  for (uint32_t jc = tid; jc < half; jc += nt) {
    const uint32_t j = jc * 2u;
    const uint64_t g = base | lut[j >> L] | (j & lowmask);
    reinterpret_cast<float4 *>(s0)[sw(j) >> 1] = *reinterpret_cast<const float4 *>(st0 + g);
    reinterpret_cast<float4 *>(s1)[sw(j) >> 1] = *reinterpret_cast<const float4 *>(st1 + g);
  }
  __syncthreads();

  for (int gi = 0; gi < a.n_groups; ++gi) {
    const OpGroup g = a.groups[gi];  // GK_REG4 only (checked on the host)
    const int b0 = g.bits[0], b1 = g.bits[1], b2 = g.bits[2], b3 = g.bits[3];
    uint32_t off[16];
#pragma unroll
    for (int c = 0; c < 16; ++c)
      off[c] = sw(((c & 1) ? (1u << b0) : 0u) | ((c & 2) ? (1u << b1) : 0u) |
                  ((c & 4) ? (1u << b2) : 0u) | ((c & 8) ? (1u << b3) : 0u));
    const uint32_t cnt = 1u << (T - 4);
    for (uint32_t i = tid; i < cnt; i += nt) {
      const uint32_t bs = sw(ins0(ins0(ins0(ins0(i, b0), b1), b2), b3));
      float2 x[16], y[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        x[c] = s0[bs ^ off[c]];
        y[c] = s1[bs ^ off[c]];
      }
      for (int k = 0; k < g.n_ops; ++k) {
        const OpSlot *sl = slots + (g.op_begin - a.op_begin + k);
        const LoweredOp op = sl->op;
        const Mat2 m = load_mat2(sl->m);
        const int cb = op.nc ? op.c0 : -1;
        if (op.slot >= 0) {
          float2 t[16];
#pragma unroll
          for (int c = 0; c < 16; ++c) t[c] = x[c];
          reg_dispatch<0>(t, gen_matrix(op.pad), cb, op.t0);
          float im = reg_im_dot(y, t);
          if (cb >= 0) {
            // rows with control = 0 are untouched by both applications -> they cancel
            Mat2 zero = gen_matrix(AG_P1);
            zero.m11 = make_float2(0.f, 0.f);
#pragma unroll
            for (int c = 0; c < 16; ++c) t[c] = x[c];
            reg_dispatch<1>(t, zero, cb, op.t0);
            im -= reg_im_dot(y, t);
          }
          im = wave_sum(im);
          if (lane == 0) ov[w * A.n_terms + op.slot] += im;
        }
        if (op.flags & LF_PERMX) { reg_dispatch<2>(x, m, cb, op.t0); reg_dispatch<2>(y, m, cb, op.t0); }
        else if (op.flags & LF_DIAG) { reg_dispatch<1>(x, m, cb, op.t0); reg_dispatch<1>(y, m, cb, op.t0); }
        else { reg_dispatch<0>(x, m, cb, op.t0); reg_dispatch<0>(y, m, cb, op.t0); }
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        s0[bs ^ off[c]] = x[c];
        s1[bs ^ off[c]] = y[c];
      }
    }
    __syncthreads();
  }
  for (uint32_t jc = tid; jc < half; jc += nt) {
    const uint32_t j = jc * 2u;
    const uint64_t g = base | lut[j >> L] | (j & lowmask);
    *reinterpret_cast<float4 *>(st0 + g) = reinterpret_cast<float4 *>(s0)[sw(j) >> 1];
    *reinterpret_cast<float4 *>(st1 + g) = reinterpret_cast<float4 *>(s1)[sw(j) >> 1];
  }
  for (int k = tid; k < A.n_terms; k += nt) {
    float v = 0.f;
    for (int i = 0; i < nw; ++i) v += ov[i * A.n_terms + k];
    A.partial[((size_t)b * gridDim.x + tile) * A.n_terms + k] = v;
  }
}

// grad[b][slot_k] = coef_k * sum_tiles partial[b][tile][k]; one block per (state, term)
__global__ void __launch_bounds__(256)
k_adj_tile_final(const float *__restrict__ partial, int n_tiles, int n_terms,
                 const int32_t *__restrict__ slot_of, const float *__restrict__ coef_of,
                 float *__restrict__ grad, int n_grad_slots) {
  __shared__ double red[16];
  const int b = blockIdx.x, k = blockIdx.y;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_tiles; i += blockDim.x)
    acc += partial[((size_t)b * n_tiles + i) * n_terms + k];
  const double tot = block_sum_d(acc, red);
  if (threadIdx.x == 0) grad[(size_t)b * n_grad_slots + slot_of[k]] = (float)(coef_of[k] * tot);
}

// ---- adjoint differentiation -------------------------------------------------------------
// lambda[b][i] = (sum_k w[b][k] (-1)^{|i & mask_k|}) psi[b][i]
__global__ void __launch_bounds__(256)
k_zsum_apply(const float4 *__restrict__ psi, float4 *__restrict__ lam, int n,
             const float *__restrict__ weights, ZMasks z, int n_obs) {
  const int b = blockIdx.y;
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const float *w = weights + (size_t)b * n_obs;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < chunks; k += stride) {
    const uint32_t i0 = (uint32_t)(k << 1);
    float d0 = 0.f, d1 = 0.f;
    for (int o = 0; o < n_obs; ++o) {
      const float wk = w[o];
      d0 += (__popc(i0 & z.mask[o]) & 1) ? -wk : wk;
      d1 += (__popc((i0 | 1u) & z.mask[o]) & 1) ? -wk : wk;
    }
    const float4 v = psi[(size_t)b * chunks + k];
    lam[(size_t)b * chunks + k] = make_float4(d0 * v.x, d0 * v.y, d1 * v.z, d1 * v.w);
  }
}

// partial[b][block] = sum_i conj(lambda_i) (X^x Z^z Pi_p psi)_i   (the phase i^n_y is applied by k_adj_final)
__global__ void __launch_bounds__(256)
k_adj_overlap(const float4 *__restrict__ psi_all, const float4 *__restrict__ lam_all, int n,
              AdjTerm<float> t, float2 *__restrict__ partial) {
  __shared__ float red[16];
  const int b = blockIdx.y;
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const float4 *psi = psi_all + (size_t)b * chunks;
  const float4 *lam = lam_all + (size_t)b * chunks;
  const uint64_t xk = t.xmask >> 1;
  const bool swap01 = t.xmask & 1u;
  float re = 0.f, im = 0.f;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < chunks; k += stride) {
    const uint32_t i0 = (uint32_t)(k << 1);
    if ((i0 & t.pmask & ~1u) != (t.pmask & ~1u)) continue;
    const float4 l = lam[k];
    float4 p = psi[k ^ xk];
    if (swap01) p = make_float4(p.z, p.w, p.x, p.y);
    // element e of this chunk: row i = i0 | e, source j = i ^ xmask
    float s0, s1;
    if (t.marks) {
      s0 = t.marks[i0];
      s1 = t.marks[i0 | 1u];
    } else {
      const uint32_t j0 = i0 ^ t.xmask, j1 = (i0 | 1u) ^ t.xmask;
      s0 = (__popc(j0 & t.zmask) & 1) ? -1.f : 1.f;
      s1 = (__popc(j1 & t.zmask) & 1) ? -1.f : 1.f;
    }
    if ((t.pmask & 1u)) s0 = 0.f;  // projector wants bit 0 = 1: even rows drop out
    re += s0 * (l.x * p.x + l.y * p.y) + s1 * (l.z * p.z + l.w * p.w);
    im += s0 * (l.x * p.y - l.y * p.x) + s1 * (l.z * p.w - l.w * p.z);
  }
  const float r = block_sum(re, red);
  const float i = block_sum(im, red);
  if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = make_float2(r, i);
}

// The 2x2 moment of a one-wire matrix gate on bit position t: partial[b][block][a * 2 + c] = sum_rest conj(lambda[a,
// rest]) psi[c, rest].  The states move as float4 = two amplitudes that differ in bit 0: position 0 lies inside one
// float4, every other position across the two float4 whose index differs in bit t - 1.
__global__ void __launch_bounds__(256)
k_adj_moment(const float4 *__restrict__ psi_all, const float4 *__restrict__ lam_all, int n, int t,
             float2 *__restrict__ partial) {
  __shared__ float red[4 * 8];
  const int b = blockIdx.y;
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  const float4 *psi = psi_all + (size_t)b * chunks;
  const float4 *lam = lam_all + (size_t)b * chunks;
  float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  if (t == 0) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < chunks; k += stride) {
      const float4 l = lam[k], p = psi[k];
      cot_accumulate(m, make_float2(l.x, l.y), make_float2(l.z, l.w), make_float2(p.x, p.y), make_float2(p.z, p.w));
    }
  } else {
    const uint64_t hb = (uint64_t)1 << (t - 1), low = hb - 1;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < (chunks >> 1); k += stride) {
      const uint64_t k0 = ((k & ~low) << 1) | (k & low), k1 = k0 | hb;
      const float4 l0 = lam[k0], l1 = lam[k1], p0 = psi[k0], p1 = psi[k1];
      cot_accumulate(m, make_float2(l0.x, l0.y), make_float2(l1.x, l1.y), make_float2(p0.x, p0.y), make_float2(p1.x, p1.y));
      cot_accumulate(m, make_float2(l0.z, l0.w), make_float2(l1.z, l1.w), make_float2(p0.z, p0.w), make_float2(p1.z, p1.w));
    }
  }
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = wave_sum(m[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wv * 8 + k] = m[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float re = 0.f, im = 0.f;
    for (int i = 0; i < 4; ++i) {  // (256 threads: four waves)
      re += red[i * 8 + threadIdx.x * 2];
      im += red[i * 8 + threadIdx.x * 2 + 1];
    }
    partial[((size_t)b * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = make_float2(re, im);
  }
}

}  // namespace

// ---- adjoint gradient: the workspace ---------------------------------------------------------------------------
static int adj_blocks(int n) {
  const uint64_t chunks = (uint64_t)1 << (n - 1);
  uint64_t b = (chunks + 256 * 8 - 1) / (256 * 8);
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return (int)b;
}
struct AdjLayout { size_t states, lam, mats, ang2, partial, fwd_ws, lds_ops, lds_terms, lds_fmats, tile_partial, total; };
// cot: complex partials per block (cot_partials)
static AdjLayout adj_layout(const qmle_plan *fwd, const qmle_plan *rev, int batch, int cot = 1) {
  AdjLayout L;
  const size_t sb = (size_t)batch * ((size_t)8 << fwd->n);
  L.states = 0;
  L.lam = sb;  // lambda DIRECTLY behind psi: one batch of 2B states for the backward gates
  L.mats = align_up(2 * sb, 256);
  L.ang2 = L.mats + ws_mats_bytes(rev, 2 * batch);
  L.partial = L.ang2 + align_up((size_t)2 * batch * (rev->n_slots ? rev->n_slots : 1) * sizeof(float), 256);
  L.fwd_ws = L.partial + align_up((size_t)batch * adj_blocks(fwd->n) * sizeof(float2) * cot, 256);
  L.lds_ops = L.fwd_ws + workspace_bytes_one(fwd, batch, QMLE_MEAS_STATE, 0) + 256;
  L.lds_terms = L.lds_ops + align_up(rev->lowered.size() * sizeof(LoweredOp) + 16, 256);
  L.lds_fmats = L.lds_terms + align_up(rev->lowered.size() * sizeof(AdjTermDev) + 16, 256);
  L.tile_partial = L.lds_fmats + ws_mats_bytes(fwd, batch) + 256;
  size_t tp = 0;  // fused tile passes: [B][tiles][terms of the stage]
  for (const Stage &st : rev->stages)
    if (st.kind == ST_TILE && !rev->whole_state_lds) {
      const size_t need = ((size_t)batch << (rev->n - st.T)) * (size_t)(st.op_end - st.op_begin) * sizeof(float);
      if (need > tp) tp = need;
    }
  L.total = L.tile_partial + align_up(tp, 256) + 256;
  return L;
}

// A checked call on its way through a route: the aligned workspace and its layout, the Z seed's position masks, the
// lowered operator of every reverse op of a cotangent request.
struct AdjCtx {
  const AdjCall<float> &c;
  char *ws;
  size_t ws_bytes;
  AdjLayout L;
  ZMasks z;
  std::vector<int> low_of;
  bool pauli() const { return c.obs.obs_terms != nullptr; }
  bool want_cot() const { return c.cot.off != nullptr; }
  hipStream_t stream() const { return (hipStream_t)c.stream; }
  // the Pauli seed's tables: behind everything the Z sweep lays out
  int seed_begin(SeedHold &seed, bool flat) const {
    return pauli_seed_begin(&seed.sd, c.fwd->n, c.batch, c.obs.obs_terms, c.obs.n_obs_terms, c.obs.n_obs, false, flat,
                            ws + L.total, ws_bytes - L.total, stream());
  }
  int zero_outputs() const {
    HIPCHK(hipMemsetAsync(c.d_grad, 0, (size_t)c.batch * c.n_grad_slots * sizeof(float), stream()));
    if (want_cot()) HIPCHK(hipMemsetAsync(c.cot.d_cot, 0, (size_t)c.batch * c.cot.stride * sizeof(float), stream()));
    return QMLE_OK;
  }
};

// Tables a route keeps on the reverse plan: uploaded when their hash `want` differs from the one stored with the
// blob.  A failed upload leaves no blob behind, so the next call uploads again.
struct BlobPiece {
  size_t off;
  const void *src;
  size_t bytes;
};
static int upload_cached(void *&blob, uint64_t &hash, uint64_t want, size_t total, std::initializer_list<BlobPiece> pieces) {
  if (blob && hash == want) return QMLE_OK;
  if (blob) (void)hipFree(blob);
  blob = nullptr;
  hipError_t err = hipMalloc(&blob, total);
  for (const BlobPiece &p : pieces)
    if (err == hipSuccess && p.bytes) err = hipMemcpy((char *)blob + p.off, p.src, p.bytes, hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (blob) (void)hipFree(blob);
    blob = nullptr;
    g_last_hip_error = (int)err;
    return QMLE_ERR_HIP;
  }
  hash = want;
  return QMLE_OK;
}

// ---- route 1, n <= 13: psi and lambda both fit in one workgroup's LDS -> a single launch ------------------------
static bool adj_lds_route(const qmle_plan *fwd, const qmle_plan *rev) {
  bool ok = fwd->whole_state_lds && fwd->n <= 13 && fwd->stages.size() == 1;
  for (const LoweredOp &o : rev->lowered) ok = ok && o.kind != LK_4Q;
  return ok;
}
// the reverse tape and its terms, in a blob owned by the reverse plan
static int adj_lds_tables(const AdjCtx &x, const LoweredOp **d_rops, const AdjTermDev **d_terms) {
  const AdjCall<float> &c = x.c;
  qmle_plan *rev = c.rev;
  const int n = rev->n, R = (int)rev->lowered.size();
  std::vector<AdjTermDev> tdev((size_t)(R ? R : 1));
  for (int r = 0; r < R; ++r) {
    const int src = rev->lowered_src[r][0];  // (one per operator: adj_check_one_source)
    const qmle_adjoint_term &t = c.terms[src];
    if (!adj_marks_in_bounds(t, n, rev->consts.size())) return QMLE_ERR_INVALID_ARG;
    tdev[r] = {t.out_slot, wires_to_pos(t.x_wires, n), wires_to_pos(t.z_wires, n), wires_to_pos(t.proj_wires, n),
               t.n_y,      t.coef,                     t.marks_off,                 x.want_cot() ? c.cot.off[src] : -1};
  }
  const uint64_t hsh = fnv1a(tdev.data(), tdev.size() * sizeof(AdjTermDev)) ^ ((uint64_t)R * 0x9E3779B97F4A7C15ull);
  const size_t ops_b = align_up((size_t)(R ? R : 1) * sizeof(LoweredOp), 256);
  const int rc = upload_cached(rev->adj_blob, rev->adj_hash, hsh, ops_b + tdev.size() * sizeof(AdjTermDev),
                               {{0, rev->lowered.data(), (size_t)R * sizeof(LoweredOp)},
                                {ops_b, tdev.data(), (size_t)R * sizeof(AdjTermDev)}});
  *d_rops = (const LoweredOp *)rev->adj_blob;
  *d_terms = (const AdjTermDev *)((char *)rev->adj_blob + ops_b);
  return rc;
}
static int adj_run_lds(const AdjCtx &x) {
  const AdjCall<float> &c = x.c;
  qmle_plan *fwd = c.fwd, *rev = c.rev;
  const int n = fwd->n;
  int rc = ensure_device_plan(fwd);
  if (rc != QMLE_OK) return rc;
  AdjLdsArgs a;
  rc = adj_lds_tables(x, &a.rev_ops, &a.terms);
  if (rc != QMLE_OK) return rc;
  float *fmats = (float *)(x.ws + x.L.lds_fmats);
  float *rmats = (float *)(x.ws + x.L.mats);
  rc = x.zero_outputs();
  if (rc == QMLE_OK) rc = launch_build_matrices(fwd, c.d_angles_fwd, fmats, c.batch, x.stream());
  if (rc == QMLE_OK) rc = launch_build_matrices(rev, c.d_angles_rev, rmats, c.batch, x.stream());
  if (rc != QMLE_OK) return rc;
  const Stage &fst = fwd->stages[0];
  a.fwd = fill_tile_args(fwd, fst, nullptr, fmats, c.d_angles_fwd, true, TM_STORE, nullptr, nullptr, 0);
  const size_t lds_base = ((size_t)16 << n) + 288 * sizeof(float);
  a.fwd.slots_in_lds = lds_base + (size_t)a.fwd.n_ops * sizeof(OpSlot) <= 160 * 1024 ? 1 : 0;
  const size_t lds = lds_base + (a.fwd.slots_in_lds ? (size_t)a.fwd.n_ops * sizeof(OpSlot) : 0);
  a.n_rev = (int)rev->lowered.size();
  a.rev_mats = rmats;
  a.rev_mat_floats = rev->mat_floats;
  a.rev_angles = c.d_angles_rev;
  a.rev_n_slots = rev->n_slots;
  a.rev_consts = rev->dev.d_consts;
  a.weights = c.d_weights;
  a.n_obs = c.obs.n_obs;
  SeedHold seed;
  if (x.pauli()) {  // word table and coefficient rows from global memory; the coefficient kernel runs first
    rc = x.seed_begin(seed, true);
    if (rc == QMLE_OK)
      rc = pauli_seed_flat(seed.sd, c.batch, c.d_weights, x.stream(), &a.pw.words, &a.pw.coef, &a.pw.n_words);
    if (rc != QMLE_OK) return rc;
  } else {
    a.z = x.z;
  }
  a.grad = c.d_grad;
  a.n_grad_slots = c.n_grad_slots;
  a.cot = (float *)c.cot.d_cot;
  a.cot_stride = c.cot.stride;
  if (FirstUse once{3}; once.first) {
    for (const void *k : {(const void *)k_adjoint_lds<false, false>, (const void *)k_adjoint_lds<true, false>,
                          (const void *)k_adjoint_lds<false, true>, (const void *)k_adjoint_lds<true, true>})
      HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    once.done();
  }
  bool has_dense4 = false;
  for (int g = fst.grp_begin; g < fst.grp_end; ++g)
    has_dense4 |= fwd->op_groups[g].kind == GK_DENSE4 || fwd->op_groups[g].kind == GK_REG4X;
  // all loops are strided, so the sweeps may use more threads than the 2^(n-4) register-tile
  // work items of the forward groups: one 64-lane wave per 256 amplitudes, at least 4 waves
  int threads = tile_threads(n);
  if (threads < 256 && n >= 8) threads = 256;
  auto *kernel = x.pauli() ? (has_dense4 ? k_adjoint_lds<true, true> : k_adjoint_lds<false, true>)
                           : (has_dense4 ? k_adjoint_lds<true, false> : k_adjoint_lds<false, false>);
  hipLaunchKernelGGL(kernel, dim3(1, c.batch), dim3(threads), lds, x.stream(), a);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

// ---- routes 2 and 3, the reverse plan stage by stage: fused tile passes (n >= 14) or one streaming pass per gate --
// The fused route's bookkeeping, cached on the reverse plan: per dev_op the stage-local index of its derivative (or
// -1) and its generator; per derivative its gradient slot and coefficient; per stage where its derivatives begin and
// how many they are.
struct FusedTables {
  const int32_t *d_term_idx = nullptr, *d_gtype = nullptr, *d_slot_of = nullptr;
  const float *d_coef_of = nullptr;
  std::vector<int> term_begin, n_terms;
};
static int adj_fused_tables(qmle_plan *rev, const qmle_adjoint_term *terms, FusedTables &ft) {
  const size_t nd = rev->dev_ops.size();
  std::vector<int32_t> term_idx(nd ? nd : 1, -1), gtype(nd ? nd : 1, 0), slot_of;
  std::vector<float> coef_of;
  for (const Stage &st : rev->stages) {
    ft.term_begin.push_back((int)slot_of.size());
    int cnt = 0;
    if (st.kind == ST_TILE) {
      if ((size_t)16 << st.T > (size_t)150 * 1024 || st.L < 1) return QMLE_ERR_UNSUPPORTED;
      for (int g = st.grp_begin; g < st.grp_end; ++g)
        if (rev->op_groups[g].kind != GK_REG4) return QMLE_ERR_UNSUPPORTED;
      for (int k = st.op_begin; k < st.op_end; ++k) {
        const int src = rev->dev_src[k];
        if (src < 0) return QMLE_ERR_INVALID_ARG;
        const qmle_adjoint_term &t = terms[src];
        if (t.out_slot < 0) continue;
        const LoweredOp &o = rev->dev_ops[k];
        // a single-target generator whose projector is exactly the gate's control
        const int nx = __builtin_popcount(t.x_wires), nz = __builtin_popcount(t.z_wires);
        if (t.marks_off >= 0 || nx > 1 || nz > 1 || (nx && nz && t.x_wires != t.z_wires)) return QMLE_ERR_UNSUPPORTED;
        if (o.kind != LK_1Q || o.nc > 1) return QMLE_ERR_UNSUPPORTED;
        term_idx[k] = cnt++;
        gtype[k] = nx && nz ? AG_Y : nx ? AG_X : nz ? AG_Z : AG_P1;
        slot_of.push_back(t.out_slot);
        coef_of.push_back(t.coef);
      }
    }
    ft.n_terms.push_back(cnt);
  }
  uint64_t hsh = fnv1a(term_idx.data(), term_idx.size() * 4);
  hsh = fnv1a(gtype.data(), gtype.size() * 4, hsh);
  hsh = fnv1a(slot_of.data(), slot_of.size() * 4, hsh);
  hsh = fnv1a(coef_of.data(), coef_of.size() * 4, hsh);
  const size_t nt_tot = slot_of.size() ? slot_of.size() : 1;
  const size_t o1 = align_up(term_idx.size() * 4, 256), o2 = o1 + align_up(gtype.size() * 4, 256),
               o3 = o2 + align_up(nt_tot * 4, 256);
  const int rc = upload_cached(rev->adjf_blob, rev->adjf_hash, hsh, o3 + align_up(nt_tot * 4, 256),
                               {{0, term_idx.data(), term_idx.size() * 4}, {o1, gtype.data(), gtype.size() * 4},
                                {o2, slot_of.data(), slot_of.size() * 4}, {o3, coef_of.data(), coef_of.size() * 4}});
  if (rc != QMLE_OK) return rc;
  ft.d_term_idx = (const int32_t *)rev->adjf_blob;
  ft.d_gtype = (const int32_t *)((char *)rev->adjf_blob + o1);
  ft.d_slot_of = (const int32_t *)((char *)rev->adjf_blob + o2);
  ft.d_coef_of = (const float *)((char *)rev->adjf_blob + o3);
  if (FirstUse once{4}; once.first) {
    HIPCHK(hipFuncSetAttribute((const void *)k_tile_adj, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    once.done();
  }
  return QMLE_OK;
}
// one fused tile pass over psi and lambda: stage `stage_i` of the reverse plan and the gradients of its gates
static int adj_launch_tile_stage(const AdjCtx &x, const Stage &st, size_t stage_i, const FusedTables &ft, float2 *psi,
                                 const float *mats, const float *ang2) {
  const AdjCall<float> &c = x.c;
  float *tile_partial = (float *)(x.ws + x.L.tile_partial);
  AdjTileArgs A;
  A.t = fill_tile_args(c.rev, st, psi, mats, ang2, false, TM_STORE, nullptr, nullptr, 0);
  A.t.slots_in_lds = 1;
  A.lam = (float2 *)(x.ws + x.L.lam);
  A.term_idx = ft.d_term_idx + st.op_begin;
  A.gtype = ft.d_gtype + st.op_begin;
  A.partial = tile_partial;
  A.n_terms = ft.n_terms[stage_i];
  const int threads = 256;
  const size_t lut_n = ((size_t)1 << (st.T - st.L)) < 4 ? 4 : ((size_t)1 << (st.T - st.L));
  const size_t lds = ((size_t)16 << st.T) + 4 * lut_n + (size_t)A.t.n_ops * sizeof(OpSlot) +
                     (size_t)(threads / kWave) * (A.n_terms ? A.n_terms : 1) * sizeof(float);
  if (lds > 160 * 1024) return QMLE_ERR_UNSUPPORTED;
  const unsigned tiles = 1u << (c.rev->n - st.T);
  hipLaunchKernelGGL(k_tile_adj, dim3(tiles, c.batch), dim3(threads), lds, x.stream(), A);
  if (A.n_terms)
    hipLaunchKernelGGL(k_adj_tile_final, dim3(c.batch, A.n_terms), dim3(256), 0, x.stream(),
                       (const float *)tile_partial, (int)tiles, A.n_terms, ft.d_slot_of + ft.term_begin[stage_i],
                       ft.d_coef_of + ft.term_begin[stage_i], c.d_grad, c.n_grad_slots);
  return QMLE_OK;
}
// the reverse plan's matrices for [psi; lambda] as one batch of 2B states (the angles of psi's half and of lambda's)
static int adj_build_pair_matrices(const AdjCall<float> &c, float *mats, float *ang2, hipStream_t stream) {
  if (c.rev->n_slots > 0) {
    const size_t ab = (size_t)c.batch * c.rev->n_slots * sizeof(float);
    HIPCHK(hipMemcpyAsync(ang2, c.d_angles_rev, ab, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync((char *)ang2 + ab, c.d_angles_rev, ab, hipMemcpyDeviceToDevice, stream));
  }
  return launch_build_matrices(c.rev, ang2, mats, 2 * c.batch, stream);
}
// psi = U_N .. U_1 |0>, lambda = (the observables) psi, zeroed outputs, and the reverse plan's matrices for [psi;
// lambda] as one batch of 2B states
static int adj_prepare_states(const AdjCtx &x, float2 *psi, float2 *lam, float *mats, float *ang2) {
  const AdjCall<float> &c = x.c;
  const int n = c.fwd->n;
  int rc = run_batch_masks(c.fwd, c.d_angles_fwd, c.batch, QMLE_MEAS_STATE, nullptr, 0, psi, x.ws + x.L.fwd_ws,
                           x.ws_bytes - x.L.fwd_ws, x.stream());
  if (rc != QMLE_OK) return rc;
  if (x.pauli()) {  // lambda = (sum of weighted words) psi
    SeedHold seed;
    rc = x.seed_begin(seed, false);
    if (rc == QMLE_OK) rc = pauli_seed_apply(seed.sd, psi, lam, c.batch, c.d_weights, x.stream());
    if (rc != QMLE_OK) return rc;
  } else {  // lambda = (sum_k w_k Z..Z_k) psi
    hipLaunchKernelGGL(k_zsum_apply, dim3(grid_for(((size_t)1 << n) / 2, 256, 4096), c.batch), dim3(256), 0, x.stream(),
                       (const float4 *)psi, (float4 *)lam, n, c.d_weights, x.z, c.obs.n_obs);
  }
  rc = x.zero_outputs();
  if (rc != QMLE_OK) return rc;
  return adj_build_pair_matrices(c, mats, ang2, x.stream());
}
// The stage loop of routes 2 and 3 on the resident states s.psi and s.lam (lambda directly behind psi): per stage the
// gradients of its gates, the matrix cotangents asked for, then the stage itself on all 2B states.  It writes only the
// gradient slots and cotangent blocks its terms name, and leaves psi and lambda in front of the reverse tape's last op.
static int adj_stage_loop(const AdjCtx &x, bool fused, const SweepView<float2> &s, const float *mats, const float *ang2) {
  const AdjCall<float> &c = x.c;
  qmle_plan *rev = c.rev;
  const int n = rev->n;
  FusedTables ft;
  if (fused) {
    const int rc = adj_fused_tables(rev, c.terms, ft);
    if (rc != QMLE_OK) return rc;
  }
  size_t si = 0;
  for (const Stage &st : rev->stages) {
    const size_t stage_i = si++;
    int rc;
    if (fused && st.kind == ST_TILE) {
      rc = adj_launch_tile_stage(x, st, stage_i, ft, s.psi, mats, ang2);
      if (rc != QMLE_OK) return rc;
      continue;
    }
    const int r = fused ? rev->dev_src[st.op_begin] : st.src_ops[0];
    if (r < 0) return QMLE_ERR_INVALID_ARG;
    const qmle_adjoint_term &t = c.terms[r];
    if (t.out_slot >= 0) {
      if (!adj_marks_in_bounds(t, n, rev->consts.size())) return QMLE_ERR_INVALID_ARG;
      adj_launch_overlap(k_adj_overlap, s, t, (const float *)rev->dev.d_consts, c.d_grad, c.n_grad_slots);
    }
    // (the operator's positions and its plain record: checked by cot_request_check)
    if (x.want_cot() && c.cot.off[r] >= 0)
      adj_launch_cotangent(k_adj_moment, s, rev->lowered[x.low_of[r]], (const float *)mats, rev->mat_floats,
                           (float *)c.cot.d_cot, c.cot.stride, c.cot.off[r]);
    rc = run_stage_inplace(rev, st, s.psi, mats, ang2, 2 * c.batch, x.stream());
    if (rc != QMLE_OK) return rc;
  }
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}
static int adj_run_stages(const AdjCtx &x, bool fused) {
  const AdjCall<float> &c = x.c;
  float *mats = (float *)(x.ws + x.L.mats);
  float *ang2 = (float *)(x.ws + x.L.ang2);
  const SweepView<float2> s = {(float2 *)(x.ws + x.L.states), (float2 *)(x.ws + x.L.lam), (float2 *)(x.ws + x.L.partial),
                               c.rev->n, adj_blocks(c.rev->n), c.batch, x.stream()};
  const int rc = adj_prepare_states(x, s.psi, s.lam, mats, ang2);
  if (rc != QMLE_OK) return rc;
  return adj_stage_loop(x, fused, s, mats, ang2);
}

// Both complex64 sweeps and their cotangent forms: the checks, the workspace, the route.
static int adjoint_run(const AdjCall<float> &c) {
  int rc = adj_check_args(c, kMaxGridY / 2);  // (psi and lambda of a sample share a launch: 2 B <= kMaxGridY)
  if (rc != QMLE_OK) return rc;
  qmle_plan *fwd = c.fwd, *rev = c.rev;
  // (the sweep applies stages to LIVE states: a schedule compiled for runs from |0..0> only is refused)
  if ((fwd->flags | rev->flags) & QMLE_PLAN_INTERNAL_ZERO_RUN) return QMLE_ERR_UNSUPPORTED;
  // rev is either a NO_FUSION plan (one streaming pass per gate) or a NO_MERGE plan (fused tile
  // passes); both keep one source gate per lowered operator
  const bool fused = (rev->flags & QMLE_PLAN_NO_MERGE) && !(rev->flags & QMLE_PLAN_NO_FUSION);
  if (!fused)
    for (const Stage &st : rev->stages)
      if (st.src_ops.size() != 1) return QMLE_ERR_INVALID_ARG;
  rc = adj_check_one_source(rev);
  if (rc != QMLE_OK) return rc;
  AdjCtx x = {c, (char *)c.d_ws, c.ws_bytes, {}, {}, {}};
  rc = x.want_cot() ? cot_request_check(rev, c.cot, x.low_of) : QMLE_OK;  // (host only: before any device work)
  if (rc != QMLE_OK) return rc;
  rc = ensure_device_plan(rev);
  if (rc != QMLE_OK) return rc;
  x.L = adj_layout(fwd, rev, c.batch, cot_partials(rev, c.cot));
  if (!align_workspace(x.ws, x.ws_bytes) || x.ws_bytes < x.L.total) return QMLE_ERR_WORKSPACE;
  rc = x.pauli() ? QMLE_OK : zmasks_fill(c.obs.wire_masks, c.obs.n_obs, fwd->n, x.z);
  if (rc != QMLE_OK) return rc;
  for (int r = 0; r < c.n_terms; ++r)
    if (!adj_slot_in_range(c.terms[r], c.n_grad_slots)) return QMLE_ERR_SLOT_RANGE;
  if (x.pauli() && x.ws_bytes - x.L.total < pauli_seed_ws_bytes(c.batch, c.obs.n_obs_terms, false))
    return QMLE_ERR_WORKSPACE;
  if (adj_lds_route(fwd, rev)) return adj_run_lds(x);
  if (fwd->n < 3) return QMLE_ERR_UNSUPPORTED;  // the per-gate streaming kernels move float4 pairs
  // the fused tile pass takes generator overlaps only: said here, not by skipping the request (the caller falls
  // back to one streaming pass per gate)
  if (fused && x.want_cot()) return QMLE_ERR_UNSUPPORTED;
  return adj_run_stages(x, fused);
}

// ---- one segment of a reverse tape on states the caller holds (qmle_adjoint_segment) ---------------------------
// No forward run, no seed, no zeroed outputs: the matrices of the 2B states, then the stage loop of the streaming
// route.  The workspace: the matrix rows, the doubled angles, the partial sums.
struct AdjSegLayout { size_t mats, ang2, partial, total; };
static AdjSegLayout adj_seg_layout(const qmle_plan *rev, int batch, int cot) {
  AdjSegLayout L;
  L.mats = 0;
  L.ang2 = ws_mats_bytes(rev, 2 * batch);
  L.partial = L.ang2 + align_up((size_t)2 * batch * (rev->n_slots ? rev->n_slots : 1) * sizeof(float), 256);
  L.total = L.partial + align_up((size_t)batch * adj_blocks(rev->n) * sizeof(float2) * cot, 256) + 256;
  return L;
}
static int adjoint_segment_run(const AdjCall<float> &c, float2 *pair) {
  qmle_plan *rev = c.rev;
  if (!rev || !pair || c.batch < 1 || c.batch > kMaxGridY / 2 || !c.terms || !c.d_grad || c.n_grad_slots < 1 || !c.d_ws ||
      c.n_terms != (int)rev->ops.size() || (rev->n_slots > 0 && !c.d_angles_rev) || (c.cot.off && !c.cot.d_cot))
    return QMLE_ERR_INVALID_ARG;
  // one streaming pass per gate on LIVE states: fused tile passes and runs from |0..0> only are other plans
  if (!(rev->flags & QMLE_PLAN_NO_FUSION) || (rev->flags & QMLE_PLAN_INTERNAL_ZERO_RUN) || rev->n < 3)
    return QMLE_ERR_UNSUPPORTED;
  for (const Stage &st : rev->stages)
    if (st.src_ops.size() != 1) return QMLE_ERR_INVALID_ARG;
  int rc = adj_check_one_source(rev);
  if (rc != QMLE_OK) return rc;
  AdjCtx x = {c, (char *)c.d_ws, c.ws_bytes, {}, {}, {}};
  rc = x.want_cot() ? cot_request_check(rev, c.cot, x.low_of) : QMLE_OK;
  if (rc != QMLE_OK) return rc;
  for (int r = 0; r < c.n_terms; ++r) {
    if (!adj_slot_in_range(c.terms[r], c.n_grad_slots)) return QMLE_ERR_SLOT_RANGE;
    if (c.terms[r].out_slot >= 0 && !adj_marks_in_bounds(c.terms[r], rev->n, rev->consts.size())) return QMLE_ERR_INVALID_ARG;
  }
  const AdjSegLayout L = adj_seg_layout(rev, c.batch, cot_partials(rev, c.cot));
  if (!align_workspace(x.ws, x.ws_bytes) || x.ws_bytes < L.total) return QMLE_ERR_WORKSPACE;
  rc = ensure_device_plan(rev);
  if (rc != QMLE_OK) return rc;
  float *mats = (float *)(x.ws + L.mats), *ang2 = (float *)(x.ws + L.ang2);
  const SweepView<float2> s = {pair, pair + ((size_t)c.batch << rev->n), (float2 *)(x.ws + L.partial), rev->n,
                               adj_blocks(rev->n), c.batch, x.stream()};
  rc = adj_build_pair_matrices(c, mats, ang2, x.stream());
  if (rc != QMLE_OK) return rc;
  return adj_stage_loop(x, false, s, mats, ang2);
}

extern "C" {

size_t qmle_adjoint_segment_workspace_bytes(const qmle_plan *rev, int batch, int two_wire) {
  if (!rev || batch < 1) return 0;
  return adj_seg_layout(rev, batch, two_wire ? 16 : 4).total + 256;
}
int qmle_adjoint_segment(qmle_plan *rev, const float *d_angles_rev, int batch, void *d_pair,
                         const qmle_adjoint_term *terms, int n_terms, float *d_grad, int n_grad_slots,
                         const int32_t *cot_off, int cot_stride, float *d_cot, void *d_ws, size_t ws_bytes,
                         qmle_stream stream) {
  return adjoint_segment_run({nullptr, rev, nullptr, d_angles_rev, batch, nullptr, {}, terms, n_terms, d_grad,
                              n_grad_slots, d_ws, ws_bytes, stream, {cot_off, cot_stride, d_cot}},
                             (float2 *)d_pair);
}

size_t qmle_adjoint_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch) {
  if (!adj_ws_query_ok(fwd, rev, batch)) return 0;
  return adj_layout(fwd, rev, batch).total + 256;
}
size_t qmle_adjoint_pauli_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch, int n_obs_terms,
                                          int n_obs) {
  if (!adj_ws_query_ok(fwd, rev, batch, 1, n_obs_terms, n_obs)) return 0;
  return adj_ws_with_seed(adj_layout(fwd, rev, batch).total, batch, n_obs_terms, false);
}
size_t qmle_adjoint_cotangent_at_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch,
                                                 int n_obs_terms, int n_obs, int two_wire) {
  if (!adj_ws_query_ok(fwd, rev, batch, 0, n_obs_terms, n_obs)) return 0;
  return adj_ws_with_seed(adj_layout(fwd, rev, batch, two_wire ? 16 : 4).total, batch, n_obs_terms, false);
}
size_t qmle_adjoint_cotangent_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch, int n_obs_terms,
                                              int n_obs) {
  return qmle_adjoint_cotangent_at_workspace_bytes(fwd, rev, batch, n_obs_terms, n_obs, 0);
}

int qmle_adjoint_gradient(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd,
                          const float *d_angles_rev, int batch, const float *d_weights,
                          const uint32_t *obs_wire_masks, int n_obs,
                          const qmle_adjoint_term *terms, int n_terms, float *d_grad,
                          int n_grad_slots, void *d_workspace, size_t workspace_bytes,
                          qmle_stream stream) {
  return adjoint_run({fwd, rev, d_angles_fwd, d_angles_rev, batch, d_weights, {obs_wire_masks, nullptr, 0, n_obs},
                      terms, n_terms, d_grad, n_grad_slots, d_workspace, workspace_bytes, stream, {}});
}

int qmle_adjoint_gradient_pauli(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd,
                                const float *d_angles_rev, int batch, const float *d_weights,
                                const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                                const qmle_adjoint_term *terms, int n_terms, float *d_grad,
                                int n_grad_slots, void *d_ws, size_t ws_bytes, qmle_stream stream) {
  return adj_entry_pauli<float>(adjoint_run, qmle_adjoint_pauli_workspace_bytes,
                                {fwd, rev, d_angles_fwd, d_angles_rev, batch, d_weights,
                                 {nullptr, obs_terms, n_obs_terms, n_obs}, terms, n_terms, d_grad, n_grad_slots, d_ws,
                                 ws_bytes, stream, {}});
}

int qmle_adjoint_cotangent_at(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd, const float *d_angles_rev,
                              int batch, const float *d_weights, const uint32_t *obs_wire_masks,
                              const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                              const qmle_adjoint_term *terms, int n_terms, float *d_grad, int n_grad_slots,
                              const int32_t *cot_off, int cot_stride, float *d_cot, void *d_ws, size_t ws_bytes,
                              qmle_stream stream) {
  return adj_entry_cotangent_at<float>(adjoint_run, qmle_adjoint_cotangent_at_workspace_bytes,
                                       {fwd, rev, d_angles_fwd, d_angles_rev, batch, d_weights,
                                        {obs_wire_masks, obs_terms, n_obs_terms, n_obs}, terms, n_terms, d_grad,
                                        n_grad_slots, d_ws, ws_bytes, stream, {cot_off, cot_stride, d_cot}});
}

int qmle_adjoint_cotangent(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd, const float *d_angles_rev,
                           int batch, const float *d_weights, const uint32_t *obs_wire_masks,
                           const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                           const qmle_adjoint_term *terms, int n_terms, float *d_grad, int n_grad_slots,
                           const int32_t *mat_out, int n_mat, float *d_cot, void *d_ws, size_t ws_bytes,
                           qmle_stream stream) {
  return adj_entry_cotangent<float>(adjoint_run, qmle_adjoint_cotangent_at_workspace_bytes,
                                    {fwd, rev, d_angles_fwd, d_angles_rev, batch, d_weights,
                                     {obs_wire_masks, obs_terms, n_obs_terms, n_obs}, terms, n_terms, d_grad,
                                     n_grad_slots, d_ws, ws_bytes, stream, {mat_out, n_mat, d_cot}});
}

}  // extern "C"

// ---- the adjoint sweep of a noisy tape on vec(rho) (qmle_adjoint_density; the sweep itself: qmle_density_dev.h) ----
// what the sweep runs between two steps: the plan's stages, one operator each
struct DensUnitF32 {
  static size_t count(const qmle_plan *p) { return p->stages.size(); }
  static int src(const qmle_plan *p, size_t k) { return p->stages[k].src_ops.size() == 1 ? p->stages[k].src_ops[0] : -1; }
  static int ensure(qmle_plan *p) { return ensure_device_plan(p); }
  static size_t mats_bytes(const qmle_plan *p, int rows) { return ws_mats_bytes(p, rows); }
  static int build(const qmle_plan *p, const float *angles, float *mats, int rows, hipStream_t stream) {
    return launch_build_matrices(p, angles, mats, rows, stream);
  }
  static int apply(qmle_plan *p, size_t k, float2 *states, const float *mats, const float *angles, int rows,
                   hipStream_t stream) {
    return run_stage_inplace(p, p->stages[k], states, mats, angles, rows, stream);
  }
};

extern "C" {

size_t qmle_adjoint_density_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch, int n_cot,
                                            int n_steps) {
  return dens_workspace_bytes<float2, DensUnitF32>(fwd, rev, batch, n_cot, n_steps);
}
int qmle_adjoint_density(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd, const float *d_angles_rev,
                         int batch, int n_cot, const float *d_weights, const uint32_t *obs_wire_masks,
                         const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                         const qmle_density_step *steps, int n_steps, const float *d_chan, int n_chan, float *d_grad,
                         int n_grad_slots, void *d_ws, size_t ws_bytes, qmle_stream stream) {
  return dens_run<float2, float, DensUnitF32>({fwd, rev, d_angles_fwd, d_angles_rev, batch, n_cot, d_weights,
                                               {obs_wire_masks, obs_terms, n_obs_terms, n_obs}, steps, n_steps, d_chan,
                                               n_chan, d_grad, n_grad_slots, d_ws, ws_bytes, stream});
}
// (both precisions walk the same tape: the stages of a NO_FUSION plan are its operators)
long long qmle_adjoint_density_transfers(const qmle_plan *fwd, const qmle_plan *rev, const qmle_density_step *steps,
                                         int n_steps, int n_cot, int f64) {
  if (f64 != 0 && f64 != 1) return QMLE_ERR_INVALID_ARG;
  return dens_transfers<DensUnitF32>(fwd, rev, steps, n_steps, n_cot);
}

}  // extern "C"
