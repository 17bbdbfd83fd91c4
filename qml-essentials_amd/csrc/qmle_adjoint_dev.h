// What the two adjoint sweeps share: qmle_adjoint.hip (complex64) and qmle_f64.hip (complex128) include this, and
// qmle_wide.hip (the moment of a three- or four-wire gate) for cot_finish_entry; no other unit does.  Device side: the kernels and helpers that are the same text in both precisions (V = float2 with
// T = float, or double2 with T = double).  Host side: a sweep's arguments, their checks, the launch pairs of the
// per-gate sweep and the bodies of the extern "C" entry points.  What differs between the precisions on purpose stays
// in the units: the kernels that move float4 against double2, the layouts, the block counts, the routes.
#pragma once
#include <climits>

#include "qmle_host.h"
#include "qmle_dev.h"

namespace {

// ---- device: sums of conj(lambda) psi ------------------------------------------------------------------------
// m[(a * 2 + c) * 2 + {0, 1}] += conj(l_a) p_c for the pair (l0, l1), (p0, p1) of one value of the other wires
template <class T, class V>
__device__ __forceinline__ void cot_accumulate(T (&m)[8], const V l0, const V l1, const V p0, const V p1) {
  m[0] += l0.x * p0.x + l0.y * p0.y; m[1] += l0.x * p0.y - l0.y * p0.x;
  m[2] += l0.x * p1.x + l0.y * p1.y; m[3] += l0.x * p1.y - l0.y * p1.x;
  m[4] += l1.x * p0.x + l1.y * p0.y; m[5] += l1.x * p0.y - l1.y * p0.x;
  m[6] += l1.x * p1.x + l1.y * p1.y; m[7] += l1.x * p1.y - l1.y * p1.x;
}
// one row of a 4x4 moment: m[c * 2 + {0, 1}] += conj(l) p_c for the four amplitudes p_c of one value of the other wires
template <class T, class V>
__device__ __forceinline__ void cot_row4(T *__restrict__ m, const V l, const V p0, const V p1, const V p2, const V p3) {
  m[0] += l.x * p0.x + l.y * p0.y; m[1] += l.x * p0.y - l.y * p0.x;
  m[2] += l.x * p1.x + l.y * p1.y; m[3] += l.x * p1.y - l.y * p1.x;
  m[4] += l.x * p2.x + l.y * p2.y; m[5] += l.x * p2.y - l.y * p2.x;
  m[6] += l.x * p3.x + l.y * p3.y; m[7] += l.x * p3.y - l.y * p3.x;
}
// Im(i^n_y (re + i im)): what a generator with n_y factors Y contributes from the overlap <lambda| X^x Z^z Pi_p |psi>
template <class T> __device__ __forceinline__ T adj_phase(int n_y, T re, T im) {
  const int q = n_y & 3;
  return q == 0 ? im : q == 1 ? re : q == 2 ? -im : -re;
}
// G = M (U^+)^T for the DIM x DIM moment M[a][c] = sum conj(lambda[a]) psi[c] taken BEHIND the gate: phi = U^+ psi is
// the state in front of it, so G[a][c] = sum conj(lambda[a]) phi[c] = sum_d M[a][d] U^+[c][d].  `ud`: the reverse
// op's own matrix (U^+), `m`: M as (re, im) pairs, row-major.
// One entry of that product: (re, im) = G[a][c].
template <int DIM, class T, class MT>
__device__ __forceinline__ void cot_finish_entry(const T *__restrict__ m, const MT *__restrict__ ud, int a, int c, T &re,
                                                 T &im) {
  re = 0, im = 0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const T mr = m[(a * DIM + d) * 2], mi = m[(a * DIM + d) * 2 + 1];
    const T ur = (T)ud[(c * DIM + d) * 2], ui = (T)ud[(c * DIM + d) * 2 + 1];
    re += mr * ur - mi * ui;
    im += mr * ui + mi * ur;
  }
}
template <int DIM, class T, class MT, class OT>
__device__ __forceinline__ void cot_finish(const T *__restrict__ m, const MT *__restrict__ ud, OT *__restrict__ out) {
#pragma unroll
  for (int a = 0; a < DIM; ++a)
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      T re, im;
      cot_finish_entry<DIM>(m, ud, a, c, re, im);
      out[(a * DIM + c) * 2] = (OT)re;
      out[(a * DIM + c) * 2 + 1] = (OT)im;
    }
}
__device__ __forceinline__ float wave_sum_any(float v) { return wave_sum(v); }
__device__ __forceinline__ double wave_sum_any(double v) { return wave_sum_d(v); }

// ---- device: what the per-gate kernels take ------------------------------------------------------------------
// the generator of one overlap; T: the scalar of the plan's constants
template <class T> struct AdjTerm {
  uint32_t xmask, zmask, pmask;  // bit positions: flipped / sign / projected onto 1
  const T *marks;                // != nullptr: G = diag(marks)
};
struct ZMasks {
  uint32_t mask[QMLE_MAX_QUBITS];  // bit-position masks of the Z (x) Z ... observables
};

// ---- device: the finishing kernels, one block per state ------------------------------------------------------
// grad[b][slot] = coef * Im(i^n_y * sum_blocks partial[b][block]), summed in double
template <class V, class T>
__global__ void __launch_bounds__(256)
k_adj_final(const V *__restrict__ partial, int n_blocks, int n_y, T coef, T *__restrict__ grad, int n_grad_slots,
            int slot) {
  __shared__ double red[16];
  const int b = blockIdx.x;
  double re = 0.0, im = 0.0;
  for (int k = threadIdx.x; k < n_blocks; k += blockDim.x) {
    const V v = partial[(size_t)b * n_blocks + k];
    re += v.x;
    im += v.y;
  }
  const double r = block_sum_d(re, red);
  const double i = block_sum_d(im, red);
  if (threadIdx.x == 0) grad[(size_t)b * n_grad_slots + slot] = (T)((double)coef * adj_phase(n_y, r, i));
}
// cot[b][off ..] = (sum_blocks partial[b][block]) (U^+)^T, summed in double; U^+ = the reverse op's 2x2 of sample b
template <class V, class T>
__global__ void __launch_bounds__(256)
k_adj_cot_final(const V *__restrict__ partial, int n_blocks, const T *__restrict__ mats, uint32_t mat_floats,
                uint32_t mat_off, T *__restrict__ cot, int cot_stride, int cot_off) {
  __shared__ double red[16];
  const int b = blockIdx.x;
  double m[8];
  for (int e = 0; e < 4; ++e) {
    double re = 0.0, im = 0.0;
    for (int k = threadIdx.x; k < n_blocks; k += blockDim.x) {
      const V v = partial[((size_t)b * n_blocks + k) * 4 + e];
      re += v.x;
      im += v.y;
    }
    m[2 * e] = block_sum_d(re, red);
    m[2 * e + 1] = block_sum_d(im, red);
  }
  if (threadIdx.x == 0)
    cot_finish<2>((const double *)m, mats + (size_t)b * mat_floats + mat_off, cot + (size_t)b * cot_stride + cot_off);
}

// The 4x4 moment of a two-wire matrix gate on bit positions (t0, t1), row = 2 bit[t0] + bit[t1] (the LK_2Q rule):
// partial[b][block][a * 4 + c] = sum_rest conj(lambda[a, rest]) psi[c, rest], one quad of each state per iteration,
// any two positions.  Plain 8- / 16-byte loads.
template <class V, class T>
__global__ void __launch_bounds__(256)
k_adj_moment2(const V *__restrict__ psi_all, const V *__restrict__ lam_all, int n, int t0, int t1,
              V *__restrict__ partial) {
  __shared__ T red[4 * 32];
  const int b = blockIdx.y;
  const V *psi = psi_all + ((size_t)b << n), *lam = lam_all + ((size_t)b << n);
  const uint64_t quads = n >= 2 ? (uint64_t)1 << (n - 2) : 0, b0 = (uint64_t)1 << t0, b1 = (uint64_t)1 << t1;
  const int plo = t0 < t1 ? t0 : t1, phi = t0 < t1 ? t1 : t0;
  T m0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m2[8] = {0, 0, 0, 0, 0, 0, 0, 0},
    m3[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t j = ins0_64(ins0_64(q, plo), phi);
    const V p0 = psi[j], p1 = psi[j | b1], p2 = psi[j | b0], p3 = psi[j | b0 | b1];
    cot_row4(m0, lam[j], p0, p1, p2, p3);
    cot_row4(m1, lam[j | b1], p0, p1, p2, p3);
    cot_row4(m2, lam[j | b0], p0, p1, p2, p3);
    cot_row4(m3, lam[j | b0 | b1], p0, p1, p2, p3);
  }
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    m0[k] = wave_sum_any(m0[k]);
    m1[k] = wave_sum_any(m1[k]);
    m2[k] = wave_sum_any(m2[k]);
    m3[k] = wave_sum_any(m3[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      red[wv * 32 + k] = m0[k];
      red[wv * 32 + 8 + k] = m1[k];
      red[wv * 32 + 16 + k] = m2[k];
      red[wv * 32 + 24 + k] = m3[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 16) {  // (256 threads: four waves)
    T re = 0, im = 0;
    for (int i = 0; i < 4; ++i) {
      re += red[i * 32 + threadIdx.x * 2];
      im += red[i * 32 + threadIdx.x * 2 + 1];
    }
    V v;
    v.x = re;
    v.y = im;
    partial[((size_t)b * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = v;
  }
}
// cot[b][off ..] = (sum_blocks partial[b][block]) (U^+)^T, summed in double; U^+ = the reverse op's 4x4 of sample b
template <class V, class T>
__global__ void __launch_bounds__(256)
k_adj_cot2_final(const V *__restrict__ partial, int n_blocks, const T *__restrict__ mats, uint32_t mat_floats,
                 uint32_t mat_off, T *__restrict__ cot, int cot_stride, int cot_off) {
  __shared__ double red[16];
  __shared__ double msum[32];
  const int b = blockIdx.x;
#pragma unroll 1
  for (int e = 0; e < 16; ++e) {
    double re = 0.0, im = 0.0;
    for (int k = threadIdx.x; k < n_blocks; k += blockDim.x) {
      const V v = partial[((size_t)b * n_blocks + k) * 16 + e];
      re += v.x;
      im += v.y;
    }
    const double r = block_sum_d(re, red);
    const double s = block_sum_d(im, red);
    if (threadIdx.x == 0) {
      msum[2 * e] = r;
      msum[2 * e + 1] = s;
    }
  }
  if (threadIdx.x == 0)
    cot_finish<4>((const double *)msum, mats + (size_t)b * mat_floats + mat_off, cot + (size_t)b * cot_stride + cot_off);
}

// ---- host: a sweep's arguments -------------------------------------------------------------------------------
// The observables of a sweep: Z-parity wire masks or a list of weighted Pauli words (obs_terms != nullptr, checked by
// the entry point); the sweeps differ in the seed alone.
struct AdjObs {
  const uint32_t *wire_masks;
  const qmle_pauli_term *obs_terms;
  int n_obs_terms, n_obs;
};
// A request for matrix cotangents beside the angle gradients: off[r] = offset, in scalars, of reverse op r's block
// inside a sample's row of `stride` scalars, or -1; a block is 8 scalars (a 2x2, re / im) for a one-wire matrix gate
// and 32 for a two-wire one.  off == nullptr: no request.
struct CotRequest {
  const int32_t *off;
  int stride;
  void *d_cot;
};
// everything an entry point hands to its sweep; T = float or double
template <class T> struct AdjCall {
  qmle_plan *fwd, *rev;
  const T *d_angles_fwd, *d_angles_rev;
  int batch;
  const T *d_weights;
  AdjObs obs;
  const qmle_adjoint_term *terms;
  int n_terms;
  T *d_grad;
  int n_grad_slots;
  void *d_ws;
  size_t ws_bytes;
  qmle_stream stream;
  CotRequest cot;
};
struct SeedHold {  // ends the Pauli seed's host plan on every way out
  PauliSeed *sd = nullptr;
  ~SeedHold() { pauli_seed_end(sd); }
};

// ---- host: argument checks, each QMLE_OK or the code to return -----------------------------------------------
// null pointers, counts and the two plans against each other; max_batch: what one launch's grid takes
template <class T> int adj_check_args(const AdjCall<T> &c, int max_batch = INT_MAX) {
  const bool pauli = c.obs.obs_terms != nullptr;
  if (!c.fwd || !c.rev || c.batch < 1 || c.batch > max_batch || !c.d_weights || (!pauli && !c.obs.wire_masks) ||
      c.obs.n_obs < 1 || (!pauli && c.obs.n_obs > QMLE_MAX_QUBITS) || !c.terms || !c.d_grad || c.n_grad_slots < 1 ||
      !c.d_ws || c.fwd->n != c.rev->n || c.n_terms != (int)c.rev->ops.size())
    return QMLE_ERR_INVALID_ARG;
  if ((c.fwd->n_slots > 0 && !c.d_angles_fwd) || (c.rev->n_slots > 0 && !c.d_angles_rev)) return QMLE_ERR_INVALID_ARG;
  return QMLE_OK;
}
// one source gate (one generator) per lowered operator of the reverse plan: NO_FUSION or NO_MERGE plans
inline int adj_check_one_source(const qmle_plan *rev) {
  for (const auto &srcs : rev->lowered_src)
    if (srcs.size() != 1) return QMLE_ERR_INVALID_ARG;
  return QMLE_OK;
}
inline bool adj_slot_in_range(const qmle_adjoint_term &t, int n_grad_slots) { return t.out_slot < n_grad_slots; }
// a diagonal generator's 2^n marks lie inside the plan's `n_consts` constants
inline bool adj_marks_in_bounds(const qmle_adjoint_term &t, int n, size_t n_consts) {
  return t.marks_off < 0 || (size_t)t.marks_off + ((size_t)1 << n) <= n_consts;
}
// <Z..Z> on wire masks (bit w = wire w) -> the kernels' position masks, or QMLE_ERR_WIRE_RANGE
inline int zmasks_fill(const uint32_t *wire_masks, int n_obs, int n, ZMasks &z) {
  z = {};
  for (int k = 0; k < n_obs; ++k) {
    if (!valid_wire_mask(wire_masks[k], n)) return QMLE_ERR_WIRE_RANGE;
    z.mask[k] = wires_to_pos(wire_masks[k], n);
  }
  return QMLE_OK;
}
inline bool cot_two_wire_op(int opcode) { return opcode == QMLE_OP_MAT2 || opcode == QMLE_OP_MAT2_ROW; }
// Does the request hold a two-wire block?  (The partial sums are then 16 complex per block, not 4.)
inline bool cot_has_two_wire(const qmle_plan *rev, const int32_t *off) {
  for (size_t r = 0; off && r < rev->ops.size(); ++r)
    if (off[r] >= 0 && cot_two_wire_op(rev->ops[r].opcode)) return true;
  return false;
}
// complex partials per block of a sweep's reductions: 1, or 4 with one-wire cotangents, or 16 with a two-wire one
inline int cot_partials(const qmle_plan *rev, const CotRequest &c) {
  return !c.off ? 1 : cot_has_two_wire(rev, c.off) ? 16 : 4;
}
// The request against the reverse tape, host only; low_of[r] <- the lowered operator of reverse op r (or -1).
inline int cot_request_check(const qmle_plan *rev, const CotRequest &c, std::vector<int> &low_of) {
  if (c.stride < 1 || !c.d_cot) return QMLE_ERR_INVALID_ARG;
  low_of.assign(rev->ops.size(), -1);
  for (size_t l = 0; l < rev->lowered_src.size(); ++l)
    if (rev->lowered_src[l].size() == 1) low_of[rev->lowered_src[l][0]] = (int)l;
  std::vector<std::pair<int64_t, int64_t>> blocks;
  for (size_t r = 0; r < rev->ops.size(); ++r) {
    if (c.off[r] < 0) continue;
    const int oc = rev->ops[r].opcode;
    const bool two = cot_two_wire_op(oc);
    if (!two && oc != QMLE_OP_MAT1 && oc != QMLE_OP_MAT1_ROW) return QMLE_ERR_UNSUPPORTED;
    const int64_t end = (int64_t)c.off[r] + (two ? 32 : 8);
    if (end > c.stride) return QMLE_ERR_SLOT_RANGE;
    blocks.emplace_back((int64_t)c.off[r], end);
    // (a flagged op that was merged into a neighbour or carries a control has no moment of its own)
    if (low_of[r] < 0 || rev->lowered[low_of[r]].kind != (two ? LK_2Q : LK_1Q) || rev->lowered[low_of[r]].nc != 0)
      return QMLE_ERR_INVALID_ARG;
  }
  std::sort(blocks.begin(), blocks.end());
  for (size_t k = 1; k < blocks.size(); ++k)
    if (blocks[k].first < blocks[k - 1].second) return QMLE_ERR_SLOT_RANGE;
  return QMLE_OK;
}
// The old form of the request, mat_out[r] = index of reverse op r's 2x2 among n_mat -> offsets 8 * index.  It
// serves one-wire matrices only and says so itself.
inline int cot_offsets_of_indices(const qmle_plan *rev, const int32_t *mat_out, int n_mat, std::vector<int32_t> &off) {
  off.assign(rev->ops.size(), -1);
  for (size_t r = 0; r < rev->ops.size(); ++r) {
    if (mat_out[r] < 0) continue;
    if (mat_out[r] >= n_mat) return QMLE_ERR_SLOT_RANGE;
    const int oc = rev->ops[r].opcode;
    if (oc != QMLE_OP_MAT1 && oc != QMLE_OP_MAT1_ROW) return QMLE_ERR_UNSUPPORTED;  // (two-wire: the _at functions)
    off[r] = 8 * mat_out[r];
  }
  return QMLE_OK;
}

// ---- host: the launch pairs of the per-gate sweep ------------------------------------------------------------
// psi, lambda and the partial sums of `bc` states in flight; nb: blocks per state of the first kernel of a pair, whose
// sums the second one finishes with one block per state
template <class V> struct SweepView {
  V *psi, *lam, *partial;
  int n, nb, bc;
  hipStream_t stream;
  dim3 final_threads() const { return dim3(nb >= 256 ? 256 : 64); }
};
// overlap + final: grad[b][t.out_slot] from the generator of `t`.  `overlap`: the unit's own kernel, which reads the
// states as S (two amplitudes per float4, or one double2)
template <class V, class T, class S>
void adj_launch_overlap(void (*overlap)(const S *, const S *, int, AdjTerm<T>, V *), const SweepView<V> &s,
                        const qmle_adjoint_term &t, const T *consts, T *grad, int n_grad_slots) {
  const AdjTerm<T> a = {wires_to_pos(t.x_wires, s.n), wires_to_pos(t.z_wires, s.n), wires_to_pos(t.proj_wires, s.n),
                        t.marks_off >= 0 ? consts + t.marks_off : nullptr};
  hipLaunchKernelGGL(overlap, dim3(s.nb, s.bc), dim3(256), 0, s.stream, (const S *)s.psi, (const S *)s.lam, s.n, a,
                     s.partial);
  hipLaunchKernelGGL((k_adj_final<V, T>), dim3(s.bc), s.final_threads(), 0, s.stream, (const V *)s.partial, s.nb,
                     t.n_y, (T)t.coef, grad, n_grad_slots, t.out_slot);
}
// moment + finish: the matrix cotangent of the plain one- or two-wire operator `lo` (cot_request_check) into
// cot[b][off ..].  `moment1`: the unit's own one-wire kernel; the two-wire one is shared.
template <class V, class T, class S>
void adj_launch_cotangent(void (*moment1)(const S *, const S *, int, int, V *), const SweepView<V> &s,
                          const LoweredOp &lo, const T *mats, uint32_t mat_floats, T *cot, int stride, int off) {
  if (lo.kind == LK_2Q) {
    hipLaunchKernelGGL((k_adj_moment2<V, T>), dim3(s.nb, s.bc), dim3(256), 0, s.stream, (const V *)s.psi,
                       (const V *)s.lam, s.n, (int)lo.t0, (int)lo.t1, s.partial);
    hipLaunchKernelGGL((k_adj_cot2_final<V, T>), dim3(s.bc), s.final_threads(), 0, s.stream, (const V *)s.partial, s.nb,
                       mats, mat_floats, lo.mat_off, cot, stride, off);
  } else {
    hipLaunchKernelGGL(moment1, dim3(s.nb, s.bc), dim3(256), 0, s.stream, (const S *)s.psi, (const S *)s.lam, s.n,
                       (int)lo.t0, s.partial);
    hipLaunchKernelGGL((k_adj_cot_final<V, T>), dim3(s.bc), s.final_threads(), 0, s.stream, (const V *)s.partial, s.nb,
                       mats, mat_floats, lo.mat_off, cot, stride, off);
  }
}

// ---- host: the extern "C" functions of both units ------------------------------------------------------------
// A workspace query's arguments; min_obs_terms: 1 where the function is for Pauli seeds only, 0 where Z seeds say 0
inline bool adj_ws_query_ok(const qmle_plan *fwd, const qmle_plan *rev, int batch, int min_obs_terms = 0,
                            int n_obs_terms = 0, int n_obs = 1) {
  return fwd && rev && batch >= 1 && n_obs_terms >= min_obs_terms && n_obs >= 1;
}
// a workspace with a Pauli seed: the layout's total, the slack for aligning it, the seed's tables for `seed_batch`
inline size_t adj_ws_with_seed(size_t layout_total, int seed_batch, int n_obs_terms, bool f64) {
  return layout_total + 256 + (n_obs_terms > 0 ? pauli_seed_ws_bytes(seed_batch, n_obs_terms, f64) : 0);
}
// `run`: the unit's sweep, int(const AdjCall<T> &); `ws_pauli` / `ws_at`: its extern "C" workspace queries
template <class T, class Run, class Ws>
int adj_entry_pauli(Run run, Ws ws_pauli, const AdjCall<T> &c) {
  if (!c.fwd || !c.rev || c.fwd->n != c.rev->n || c.batch < 1 || !c.d_weights || !c.d_ws) return QMLE_ERR_INVALID_ARG;
  const int rc = pauli_seed_check(c.fwd->n, c.obs.obs_terms, c.obs.n_obs_terms, c.obs.n_obs);
  if (rc != QMLE_OK) return rc;
  if (c.ws_bytes < ws_pauli(c.fwd, c.rev, c.batch, c.obs.n_obs_terms, c.obs.n_obs)) return QMLE_ERR_INVALID_ARG;
  return run(c);
}
// what both cotangent entry points ask of their arguments first; c.cot holds the request in the caller's form
template <class T> bool adj_cot_args_ok(const AdjCall<T> &c) {
  return c.fwd && c.rev && c.fwd->n == c.rev->n && c.batch >= 1 && c.d_weights && c.d_ws && c.cot.off && c.cot.d_cot &&
         c.cot.stride >= 1 && c.n_terms == (int)c.rev->ops.size() &&
         (c.obs.wire_masks != nullptr) != (c.obs.obs_terms != nullptr);
}
template <class T, class Run, class Ws>
int adj_entry_cotangent_at(Run run, Ws ws_at, AdjCall<T> c) {
  if (!adj_cot_args_ok(c)) return QMLE_ERR_INVALID_ARG;
  if (c.obs.obs_terms) {
    const int rc = pauli_seed_check(c.fwd->n, c.obs.obs_terms, c.obs.n_obs_terms, c.obs.n_obs);
    if (rc != QMLE_OK) return rc;
  } else {
    c.obs.n_obs_terms = 0;
  }
  if (c.ws_bytes < ws_at(c.fwd, c.rev, c.batch, c.obs.n_obs_terms, c.obs.n_obs, cot_has_two_wire(c.rev, c.cot.off)))
    return QMLE_ERR_INVALID_ARG;
  return run(c);
}
// the form with one index per 2x2, c.cot = {mat_out, n_mat, d_cot}: offsets 8 * index into rows of 8 * n_mat scalars
template <class T, class Run, class Ws>
int adj_entry_cotangent(Run run, Ws ws_at, AdjCall<T> c) {
  // (the argument checks of the function above first, so that a call that is bad in two ways keeps its code)
  if (!adj_cot_args_ok(c)) return QMLE_ERR_INVALID_ARG;
  std::vector<int32_t> off;
  const int rc = cot_offsets_of_indices(c.rev, c.cot.off, c.cot.stride, off);
  if (rc != QMLE_OK) return rc;
  c.cot = {off.data(), 8 * c.cot.stride, c.cot.d_cot};
  return adj_entry_cotangent_at(run, ws_at, c);
}

}  // namespace
