// The adjoint sweep of a NOISY tape on vec(rho): qmle_adjoint_density (qmle_adjoint.hip, complex64) and
// qmle_adjoint_density_f64 (qmle_f64.hip, complex128) are this text in two precisions (V = float2 with T = float, or
// double2 with T = double); no other unit includes it.  DESIGN 6.19.
//
// A channel has no usable inverse, so the forward states are KEPT and only the observable moves backwards:
//   forward   checkpoint k+1 = (channels of step k) (U (x) conj U) checkpoint k        k_dens_fwd, out of place
//   seed      lambda = vec(sum_k w_k O_k)                                               k_dens_seed_z / k_dens_seed_pauli
//   backward  lambda' = (channels)^+ lambda;  v_mid = (U (x) conj U) checkpoint k;
//             dC/dtheta = coef Im i^n_y <lambda'| G_ket |v_mid>;  lambda = (U (x) conj U)^+ lambda'     k_dens_bwd
// A STEP is one parametrised source gate (its ket and its bra operator) and the channels behind it on the same wires,
// premultiplied by the host into one superoperator: 2 or 4 bit positions of the 2n-wire index, 4 or 16 amplitudes per
// work item in registers.  Everything between two steps runs through the unit's one-operator-per-pass machinery
// (DensUnitF32 / DensUnitF64 in the units): forward in place on the newest checkpoint, backward on lambda alone.
#pragma once
#include <climits>

#include "qmle_host.h"
#include "qmle_dev.h"
#include "qmle_adjoint_dev.h"

namespace {

// ---- device: complex arithmetic in both precisions -----------------------------------------------------------
__device__ __forceinline__ float2 dz_mul(float2 a, float2 b) { return cmul(a, b); }
__device__ __forceinline__ float2 dz_fma(float2 a, float2 b, float2 c) { return cfma(a, b, c); }
__device__ __forceinline__ double2 dz_mul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 dz_fma(double2 a, double2 b, double2 c) {
  return make_double2(fma(a.x, b.x, fma(-a.y, b.y, c.x)), fma(a.x, b.y, fma(a.y, b.x, c.y)));
}
template <class V> __device__ __forceinline__ V dz_conj(V a) {
  a.y = -a.y;
  return a;
}
template <class V, class S> __device__ __forceinline__ V dz_make(S re, S im) {
  V v;
  v.x = (decltype(v.x))re;
  v.y = (decltype(v.x))im;
  return v;
}
__device__ __forceinline__ float dens_block_sum(float v, float *red) { return block_sum(v, red); }
__device__ __forceinline__ double dens_block_sum(double v, double *red) { return block_sum_d(v, red); }

// ---- device: a step -------------------------------------------------------------------------------------------
// Local index l of a step's 2^NB amplitudes: bit k of l is bit position pos[k] of the register index, pos ascending.
// The step's wires in ascending order are its ket wires and then its bra wires, so the bra wires are the low half of
// l and the ket wires the high half: l = ket * d + bra, d = 2^(NB / 2).
struct DensStepDev {
  int n;             // wires of the doubled register
  int pos[4];        // ascending bit positions (NB of them)
  int opcode;        // the source gate
  int swap;          // a two-wire gate whose first wire is the higher one
  int slot, n_slots; // its angle: column `slot` of a table row of n_slots columns
  int batch;         // samples: row r of lambda reads checkpoint row r % batch
  uint32_t gx, gz, gp;  // the generator on local bits: flipped / sign / projected onto 1 (k_adj_overlap's rule)
};

// U of the source gate on its own wires, in ASCENDING wire order (row = 2 * lower wire + higher wire), from the
// sample's angle; evaluated in fp64 like the plan's matrix builder (qmle_matrices.h restated for one gate).
template <class V, int NB>
__device__ __forceinline__ void dens_unitary(const DensStepDev &a, double th, V (&u)[1 << NB]) {
  constexpr int d = 1 << (NB / 2);
  double s, c;
  sincos(0.5 * th, &s, &c);
  const V z = dz_make<V>(0.0, 0.0), one = dz_make<V>(1.0, 0.0);
  V m00 = one, m01 = z, m10 = z, m11 = one;  // the 2x2 of a one-wire gate or of a controlled gate's target
  switch (a.opcode) {
    case QMLE_OP_RX: case QMLE_OP_CRX: m00 = m11 = dz_make<V>(c, 0.0); m01 = m10 = dz_make<V>(0.0, -s); break;
    case QMLE_OP_RY: case QMLE_OP_CRY: m00 = m11 = dz_make<V>(c, 0.0); m01 = dz_make<V>(-s, 0.0); m10 = dz_make<V>(s, 0.0); break;
    case QMLE_OP_RZ: case QMLE_OP_CRZ: m00 = dz_make<V>(c, -s); m11 = dz_make<V>(c, s); break;
    case QMLE_OP_CPHASE: {
      double sp, cp;
      sincos(th, &sp, &cp);
      m11 = dz_make<V>(cp, sp);
      break;
    }
    default: break;
  }
  if constexpr (NB == 2) {
    u[0] = m00; u[1] = m01; u[2] = m10; u[3] = m11;
  } else {
    V m[16];  // gate order: row = 2 * first wire + second wire
#pragma unroll
    for (int e = 0; e < 16; ++e) m[e] = z;
    const V cc = dz_make<V>(c, 0.0), ms = dz_make<V>(0.0, -s), ps = dz_make<V>(0.0, s);
    switch (a.opcode) {
      case QMLE_OP_RXX: m[0] = m[5] = m[10] = m[15] = cc; m[3] = m[6] = m[9] = m[12] = ms; break;
      case QMLE_OP_RYY: m[0] = m[5] = m[10] = m[15] = cc; m[3] = m[12] = ps; m[6] = m[9] = ms; break;
      case QMLE_OP_RZZ: m[0] = m[15] = dz_make<V>(c, -s); m[5] = m[10] = dz_make<V>(c, s); break;
      case QMLE_OP_RZX: m[0] = m[5] = m[10] = m[15] = cc; m[1] = m[4] = ms; m[11] = m[14] = ps; break;
      default:  // control = first wire
        m[0] = m[5] = one; m[10] = m00; m[11] = m01; m[14] = m10; m[15] = m11; break;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int cq = 0; cq < 4; ++cq) {
        const int rs = ((r & 1) << 1) | (r >> 1), cs = ((cq & 1) << 1) | (cq >> 1);
        u[r * d + cq] = a.swap ? m[rs * 4 + cs] : m[r * 4 + cq];
      }
  }
}

template <int NB> __device__ __forceinline__ uint64_t dens_base(uint64_t i, const int (&pos)[4]) {
#pragma unroll
  for (int k = 0; k < NB; ++k) i = ins0_64(i, pos[k]);
  return i;
}
template <int NB> __device__ __forceinline__ uint64_t dens_off(int l, const int (&pos)[4]) {
  uint64_t o = 0;
#pragma unroll
  for (int k = 0; k < NB; ++k)
    if ((l >> k) & 1) o |= (uint64_t)1 << pos[k];
  return o;
}
// PAIR (complex64 with bit position 0 among the step's): local neighbours l, l + 1 are one float4
template <class V, int NB, bool PAIR>
__device__ __forceinline__ void dens_load(const V *__restrict__ s, uint64_t base, const int (&pos)[4], V (&x)[1 << NB]) {
  if constexpr (PAIR) {
#pragma unroll
    for (int l = 0; l < (1 << NB); l += 2) {
      const float4 q = *reinterpret_cast<const float4 *>(s + (base | dens_off<NB>(l, pos)));
      x[l] = make_float2(q.x, q.y);
      x[l + 1] = make_float2(q.z, q.w);
    }
  } else {
#pragma unroll
    for (int l = 0; l < (1 << NB); ++l) x[l] = s[base | dens_off<NB>(l, pos)];
  }
}
template <class V, int NB, bool PAIR>
__device__ __forceinline__ void dens_store(V *__restrict__ s, uint64_t base, const int (&pos)[4], const V (&x)[1 << NB]) {
  if constexpr (PAIR) {
#pragma unroll
    for (int l = 0; l < (1 << NB); l += 2)
      *reinterpret_cast<float4 *>(s + (base | dens_off<NB>(l, pos))) = make_float4(x[l].x, x[l].y, x[l + 1].x, x[l + 1].y);
  } else {
#pragma unroll
    for (int l = 0; l < (1 << NB); ++l) s[base | dens_off<NB>(l, pos)] = x[l];
  }
}
// x <- (U (x) conj U) x, or with DAG its conjugate transpose (U^+ on the ket half, U^T on the bra half)
template <class V, int NB, bool DAG>
__device__ __forceinline__ void dens_gate(V (&x)[1 << NB], const V (&u)[1 << NB]) {
  constexpr int d = 1 << (NB / 2);
  V y[1 << NB];
#pragma unroll
  for (int k = 0; k < d; ++k)
#pragma unroll
    for (int b = 0; b < d; ++b) {
      V acc = dz_mul(DAG ? dz_conj(u[0 * d + k]) : u[k * d + 0], x[0 * d + b]);
#pragma unroll
      for (int j = 1; j < d; ++j) acc = dz_fma(DAG ? dz_conj(u[j * d + k]) : u[k * d + j], x[j * d + b], acc);
      y[k * d + b] = acc;
    }
#pragma unroll
  for (int k = 0; k < d; ++k)
#pragma unroll
    for (int b = 0; b < d; ++b) {
      V acc = dz_mul(DAG ? u[0 * d + b] : dz_conj(u[b * d + 0]), y[k * d + 0]);
#pragma unroll
      for (int j = 1; j < d; ++j) acc = dz_fma(DAG ? u[j * d + b] : dz_conj(u[b * d + j]), y[k * d + j], acc);
      x[k * d + b] = acc;
    }
}
// x <- C x for the step's superoperator C ([2^NB][2^NB][re, im], wave-uniform reads), or with DAG x <- C^+ x
template <class V, class T, int NB, bool DAG>
__device__ __forceinline__ void dens_chan(V (&x)[1 << NB], const T *__restrict__ cm) {
  constexpr int D = 1 << NB;
  V y[D];
#pragma unroll
  for (int r = 0; r < D; ++r) {
    V acc = dz_make<V>(0.0, 0.0);
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const int e = DAG ? c * D + r : r * D + c;
      const V m = dz_make<V>(cm[2 * e], DAG ? -cm[2 * e + 1] : cm[2 * e + 1]);
      acc = dz_fma(m, x[c], acc);
    }
    y[r] = acc;
  }
#pragma unroll
  for (int r = 0; r < D; ++r) x[r] = y[r];
}

// forward step: checkpoint k -> checkpoint k + 1, one state per grid row
template <class V, class T, int NB, bool PAIR>
__global__ void __launch_bounds__(256)
k_dens_fwd(const V *__restrict__ src_all, V *__restrict__ dst_all, const T *__restrict__ angles,
           const T *__restrict__ chan, const DensStepDev a) {
  const int b = blockIdx.y;
  const V *src = src_all + ((size_t)b << a.n);
  V *dst = dst_all + ((size_t)b << a.n);
  V u[1 << NB];
  dens_unitary<V, NB>(a, (double)angles[(size_t)b * a.n_slots + a.slot], u);
  const uint64_t items = (uint64_t)1 << (a.n - NB), stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
    const uint64_t base = dens_base<NB>(i, a.pos);
    V x[1 << NB];
    dens_load<V, NB, PAIR>(src, base, a.pos, x);
    dens_gate<V, NB, false>(x, u);
    if (chan) dens_chan<V, T, NB, false>(x, chan);
    dens_store<V, NB, PAIR>(dst, base, a.pos, x);
  }
}

// backward step: lambda <- (step)^+ lambda and partial[row][block] = sum conj(lambda') (X^x Z^z Pi_p v_mid), the
// sums k_adj_final finishes (phase i^n_y, coefficient); one row of lambda per grid row
template <class V, class T, int NB, bool PAIR>
__global__ void __launch_bounds__(256)
k_dens_bwd(const V *__restrict__ ckpt_all, V *__restrict__ lam_all, const T *__restrict__ angles,
           const T *__restrict__ chan, const DensStepDev a, V *__restrict__ partial) {
  __shared__ T red[16];
  constexpr int D = 1 << NB;
  const int row = blockIdx.y, b = row % a.batch;
  const V *ck = ckpt_all + ((size_t)b << a.n);
  V *lam = lam_all + ((size_t)row << a.n);
  V u[D];
  dens_unitary<V, NB>(a, (double)angles[(size_t)b * a.n_slots + a.slot], u);
  T re = 0, im = 0;
  const uint64_t items = (uint64_t)1 << (a.n - NB), stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
    const uint64_t base = dens_base<NB>(i, a.pos);
    V x[D], w[D];
    dens_load<V, NB, PAIR>(lam, base, a.pos, x);
    if (chan) dens_chan<V, T, NB, true>(x, chan);
    dens_load<V, NB, PAIR>(ck, base, a.pos, w);
    dens_gate<V, NB, false>(w, u);
    // w[l] <- v_mid[l ^ gx]: the generator sits on the ket half, local bits NB / 2 .. NB - 1
#pragma unroll
    for (int kb = NB / 2; kb < NB; ++kb)
      if ((a.gx >> kb) & 1u) {
#pragma unroll
        for (int l = 0; l < D; ++l)
          if (!((l >> kb) & 1)) {
            const V t = w[l];
            w[l] = w[l | (1 << kb)];
            w[l | (1 << kb)] = t;
          }
      }
#pragma unroll
    for (int l = 0; l < D; ++l) {
      const bool on = ((uint32_t)l & a.gp) == a.gp;
      const T sg = !on ? (T)0 : (__popc(((uint32_t)l ^ a.gx) & a.gz) & 1) ? (T)-1 : (T)1;
      re += sg * (x[l].x * w[l].x + x[l].y * w[l].y);
      im += sg * (x[l].x * w[l].y - x[l].y * w[l].x);
    }
    dens_gate<V, NB, true>(x, u);
    dens_store<V, NB, PAIR>(lam, base, a.pos, x);
  }
  const T r = dens_block_sum(re, red);
  const T m = dens_block_sum(im, red);
  if (threadIdx.x == 0) partial[(size_t)row * gridDim.x + blockIdx.x] = dz_make<V>(r, m);
}

// ---- device: checkpoint 0 and the seeds -----------------------------------------------------------------------
template <class V> __global__ void __launch_bounds__(256) k_dens_init(V *__restrict__ states, int n) {
  const uint64_t D = (uint64_t)1 << n;
  V *s = states + ((size_t)blockIdx.y << n);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < D; i += (uint64_t)gridDim.x * blockDim.x)
    s[i] = dz_make<V>(i == 0 ? 1.0 : 0.0, 0.0);
}
// lambda[r][i * 2^ns + j] = (i == j) sum_k w[r][k] (-1)^{|i & mask_k|}; ns system wires, masks as bit positions of i
template <class V, class T>
__global__ void __launch_bounds__(256)
k_dens_seed_z(V *__restrict__ lam_all, int ns, const T *__restrict__ weights, ZMasks z, int n_obs) {
  const int r = blockIdx.y;
  const uint64_t D = (uint64_t)1 << (2 * ns), low = ((uint64_t)1 << ns) - 1;
  const T *w = weights + (size_t)r * n_obs;
  V *lam = lam_all + ((size_t)r << (2 * ns));
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < D; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t i = (uint32_t)(e >> ns), j = (uint32_t)(e & low);
    T dsum = 0;
    if (i == j)
      for (int o = 0; o < n_obs; ++o) dsum += (__popc(i & z.mask[o]) & 1) ? -w[o] : w[o];
    lam[e] = dz_make<V>(dsum, (T)0);
  }
}
// The Pauli seed: lambda = vec(sum_t w[r][obs_t] coef_t P_t), P[i][i ^ x] = i^ny (-1)^{|(i ^ x) & z|} (the rule of
// qmle_apply_pauli_sum).  lambda is zeroed first; one work item per row i of Lambda walks the terms, each of which owns
// entry (i, i ^ x) of that row, so no two work items meet.
constexpr int kDensMaxSeedTerms = 96;
template <class T> struct DensSeedTerms {
  uint32_t x[kDensMaxSeedTerms], z[kDensMaxSeedTerms];  // bit positions of the system index
  int32_t obs[kDensMaxSeedTerms];
  T coef[kDensMaxSeedTerms];
  int n;
};
template <class V, class T>
__global__ void __launch_bounds__(256)
k_dens_seed_pauli(V *__restrict__ lam_all, int ns, const T *__restrict__ weights, int n_obs, const DensSeedTerms<T> s) {
  const int r = blockIdx.y;
  const uint32_t rows = 1u << ns;
  const T *w = weights + (size_t)r * n_obs;
  V *lam = lam_all + ((size_t)r << (2 * ns));
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += gridDim.x * blockDim.x)
    for (int t = 0; t < s.n; ++t) {
      const uint32_t j = i ^ s.x[t];
      const T c = ((__popc(j & s.z[t]) & 1) ? -s.coef[t] : s.coef[t]) * w[s.obs[t]];
      const int q = __popc(s.x[t] & s.z[t]) & 3;  // i^ny
      V &e = lam[((uint64_t)i << ns) | j];
      if (q == 0) e.x += c;
      else if (q == 1) e.y += c;
      else if (q == 2) e.x -= c;
      else e.y -= c;
    }
}

// ---- host: a call ---------------------------------------------------------------------------------------------
template <class T> struct DensCall {
  qmle_plan *fwd, *rev;
  const T *d_angles_fwd, *d_angles_rev;  // [batch][fwd slots]; [n_cot * batch][rev slots]
  int batch, n_cot;
  const T *d_weights;                    // [n_cot * batch][n_obs]
  AdjObs obs;
  const qmle_density_step *steps;
  int n_steps;
  const T *d_chan;
  int n_chan;                            // scalars in d_chan
  T *d_grad;
  int n_grad_slots;
  void *d_ws;
  size_t ws_bytes;
  qmle_stream stream;
};
// blocks per state of a step kernel (and partial sums per row of the backward one)
inline int dens_blocks(int n, int nb) {
  const uint64_t items = (uint64_t)1 << (n - nb);
  uint64_t b = (items + 256 * 4 - 1) / (256 * 4);
  return (int)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}
inline int dens_step_bits(const qmle_density_step &s) { return s.wires[1] >= 0 ? 4 : 2; }
// A step against the register (ns system wires) and the two tapes: QMLE_OK or the code to return
inline int dens_check_step(const qmle_density_step &s, int ns, int n_fwd_ops, int n_rev_ops, int fwd_slots, int n_chan,
                           int n_grad_slots) {
  const bool two = s.wires[1] >= 0;
  switch (s.opcode) {
    case QMLE_OP_RX: case QMLE_OP_RY: case QMLE_OP_RZ:
      if (two) return QMLE_ERR_WIRE_COUNT;
      break;
    case QMLE_OP_CRX: case QMLE_OP_CRY: case QMLE_OP_CRZ: case QMLE_OP_CPHASE: case QMLE_OP_RXX: case QMLE_OP_RYY:
    case QMLE_OP_RZZ: case QMLE_OP_RZX:
      if (!two) return QMLE_ERR_WIRE_COUNT;
      break;
    default: return QMLE_ERR_UNSUPPORTED;
  }
  if (s.wires[0] < 0 || s.wires[0] >= ns || (two && s.wires[1] >= ns)) return QMLE_ERR_WIRE_RANGE;
  if (two && s.wires[0] == s.wires[1]) return QMLE_ERR_DUPLICATE_WIRES;
  if (s.angle_slot < 0 || s.angle_slot >= fwd_slots) return QMLE_ERR_SLOT_RANGE;
  if (s.term.out_slot < 0 || s.term.out_slot >= n_grad_slots) return QMLE_ERR_SLOT_RANGE;
  const int dim = two ? 16 : 4;
  if (s.chan_off < -1 || (s.chan_off >= 0 && (int64_t)s.chan_off + 2 * dim * dim > n_chan)) return QMLE_ERR_INVALID_ARG;
  if (s.fwd_first < 0 || s.fwd_count < 1 || s.fwd_first + s.fwd_count > n_fwd_ops || s.rev_first < 0 ||
      s.rev_count < 1 || s.rev_first + s.rev_count > n_rev_ops)
    return QMLE_ERR_INVALID_ARG;
  const uint32_t ket = (1u << s.wires[0]) | (two ? 1u << s.wires[1] : 0u);
  if (((s.term.x_wires | s.term.z_wires | s.term.proj_wires) & ~ket) || s.term.marks_off >= 0) return QMLE_ERR_INVALID_ARG;
  return QMLE_OK;
}
// the kernels' view of a step
inline DensStepDev dens_step_dev(const qmle_density_step &s, int n, int batch, int n_slots) {
  const int ns = n / 2;
  const bool two = s.wires[1] >= 0;
  DensStepDev a = {};
  a.n = n;
  a.opcode = s.opcode;
  a.swap = two && s.wires[0] > s.wires[1];
  a.slot = s.angle_slot;
  a.n_slots = n_slots;
  a.batch = batch;
  // wires ascending: ket (lower first), then bra; local bit NB - 1 - index, positions ascending with the local bit
  int wires[4], nb = two ? 4 : 2;
  if (two) {
    const int lo = std::min(s.wires[0], s.wires[1]), hi = std::max(s.wires[0], s.wires[1]);
    wires[0] = lo; wires[1] = hi; wires[2] = lo + ns; wires[3] = hi + ns;
  } else {
    wires[0] = s.wires[0]; wires[1] = s.wires[0] + ns;
  }
  for (int k = 0; k < nb; ++k) a.pos[k] = n - 1 - wires[nb - 1 - k];
  auto local = [&](uint32_t mask) {
    uint32_t m = 0;
    for (int k = 0; k < nb; ++k)
      if (wires[k] < ns && (mask >> wires[k]) & 1u) m |= 1u << (nb - 1 - k);
    return m;
  };
  a.gx = local(s.term.x_wires);
  a.gz = local(s.term.z_wires);
  a.gp = local(s.term.proj_wires);
  return a;
}

// What the unit's one-operator-per-pass machinery offers the sweep (its `Unit` parameter): `count(p)` walk entries in tape order,
// `src(p, k)` the tape op of entry k (or -1), `ensure`, `mats_bytes`, `build` (the matrix rows of `rows` states from
// their angle rows) and `apply` (entry k in place on `rows` resident states).
// The walk of one plan: entry k runs unless its op belongs to a step; `first_of[op]` = the step that begins there.
struct DensWalk {
  std::vector<int> step_of, first_of;  // per tape op: the step that replaces it / that begins with it, or -1
};
inline int dens_walk(const qmle_density_step *steps, int n_steps, int n_ops, bool rev, DensWalk &w) {
  w.step_of.assign((size_t)n_ops, -1);
  w.first_of.assign((size_t)n_ops, -1);
  for (int s = 0; s < n_steps; ++s) {
    const int first = rev ? steps[s].rev_first : steps[s].fwd_first, cnt = rev ? steps[s].rev_count : steps[s].fwd_count;
    for (int k = first; k < first + cnt; ++k) {
      if (w.step_of[k] >= 0) return QMLE_ERR_INVALID_ARG;  // two steps share an op
      w.step_of[k] = s;
    }
    w.first_of[first] = s;
  }
  return QMLE_OK;
}
// the modelled state-sized reads and writes of a call, per sample: forward once, backward n_cot times
template <class Unit>
int64_t dens_transfers(const qmle_plan *fwd, const qmle_plan *rev, const qmle_density_step *steps, int n_steps,
                       int n_cot) {
  if (!fwd || !rev || n_steps < 0 || (n_steps && !steps) || n_cot < 1) return QMLE_ERR_INVALID_ARG;
  for (int s = 0; s < n_steps; ++s)
    if (steps[s].fwd_first < 0 || steps[s].fwd_count < 1 || steps[s].fwd_first + steps[s].fwd_count > (int)fwd->ops.size() ||
        steps[s].rev_first < 0 || steps[s].rev_count < 1 || steps[s].rev_first + steps[s].rev_count > (int)rev->ops.size())
      return QMLE_ERR_INVALID_ARG;
  DensWalk wf, wr;
  if (dens_walk(steps, n_steps, (int)fwd->ops.size(), false, wf) != QMLE_OK ||
      dens_walk(steps, n_steps, (int)rev->ops.size(), true, wr) != QMLE_OK)
    return QMLE_ERR_INVALID_ARG;
  int64_t f = 1, b = 1;  // checkpoint 0 written; the seed written
  for (size_t k = 0; k < Unit::count(fwd); ++k) {
    const int op = Unit::src(fwd, k);
    if (op < 0) return QMLE_ERR_INVALID_ARG;
    f += wf.step_of[op] < 0 ? 2 : wf.first_of[op] >= 0 ? 2 : 0;
  }
  int left = n_steps;  // the backward walk ends behind the first step of the tape
  for (size_t k = 0; k < Unit::count(rev) && left > 0; ++k) {
    const int op = Unit::src(rev, k);
    if (op < 0) return QMLE_ERR_INVALID_ARG;
    if (wr.step_of[op] < 0) b += 2;
    else if (wr.first_of[op] >= 0) { b += 3; --left; }
  }
  return f + (int64_t)n_cot * b;
}

struct DensLayout { size_t fmats, rmats, partial, ckpt, lam, total; };
template <class V, class Unit>
DensLayout dens_layout(const qmle_plan *fwd, const qmle_plan *rev, int batch, int n_cot, int n_steps) {
  DensLayout L;
  const size_t rows = (size_t)batch * n_cot, state = sizeof(V) << fwd->n;
  L.fmats = 0;
  L.rmats = align_up(L.fmats + Unit::mats_bytes(fwd, batch), 256);
  L.partial = align_up(L.rmats + Unit::mats_bytes(rev, (int)rows), 256);
  L.ckpt = L.partial + align_up(rows * 1024 * sizeof(V), 256);
  L.lam = L.ckpt + align_up((size_t)(n_steps + 1) * batch * state, 256);
  L.total = L.lam + align_up(rows * state, 256) + 256;
  return L;
}
template <class V, class Unit>
size_t dens_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch, int n_cot, int n_steps) {
  if (!fwd || !rev || fwd->n != rev->n || batch < 1 || n_cot < 1 || n_steps < 0 || (int64_t)batch * n_cot > kMaxGridY)
    return 0;
  return dens_layout<V, Unit>(fwd, rev, batch, n_cot, n_steps).total + 256;
}

// PAIR: complex64 with bit position 0 among the step's
template <class V, class T, int NB>
void dens_launch_fwd(const V *src, V *dst, const T *angles, const T *chan, const DensStepDev &a, hipStream_t stream) {
  const dim3 grid(dens_blocks(a.n, NB), a.batch);
  if constexpr (sizeof(T) == 4) {
    if (a.pos[0] == 0) {
      hipLaunchKernelGGL((k_dens_fwd<V, T, NB, true>), grid, dim3(256), 0, stream, src, dst, angles, chan, a);
      return;
    }
  }
  hipLaunchKernelGGL((k_dens_fwd<V, T, NB, false>), grid, dim3(256), 0, stream, src, dst, angles, chan, a);
}
template <class V, class T, int NB>
void dens_launch_bwd(const V *ck, V *lam, const T *angles, const T *chan, const DensStepDev &a, int rows, V *partial,
                     hipStream_t stream) {
  const dim3 grid(dens_blocks(a.n, NB), rows);
  if constexpr (sizeof(T) == 4) {
    if (a.pos[0] == 0) {
      hipLaunchKernelGGL((k_dens_bwd<V, T, NB, true>), grid, dim3(256), 0, stream, ck, lam, angles, chan, a, partial);
      return;
    }
  }
  hipLaunchKernelGGL((k_dens_bwd<V, T, NB, false>), grid, dim3(256), 0, stream, ck, lam, angles, chan, a, partial);
}

// The sweep: checks (all before any device work), the workspace, forward with checkpoints, seed, backward.
template <class V, class T, class Unit> int dens_run(const DensCall<T> &c) {
  const bool pauli = c.obs.obs_terms != nullptr;
  if (!c.fwd || !c.rev || c.fwd->n != c.rev->n || c.batch < 1 || c.n_cot < 1 || (int64_t)c.batch * c.n_cot > kMaxGridY ||
      !c.d_weights || c.obs.n_obs < 1 || c.n_steps < 0 || (c.n_steps && !c.steps) || !c.d_grad || c.n_grad_slots < 1 ||
      !c.d_ws || c.n_chan < 0 || (c.n_chan && !c.d_chan))
    return QMLE_ERR_INVALID_ARG;
  if ((c.obs.wire_masks != nullptr) == pauli) return QMLE_ERR_INVALID_ARG;  // exactly one seed
  qmle_plan *fwd = c.fwd, *rev = c.rev;
  const int n = fwd->n, ns = n / 2, rows = c.batch * c.n_cot;
  if (n < 4 || (n & 1)) return QMLE_ERR_INVALID_ARG;
  if ((fwd->n_slots > 0 && !c.d_angles_fwd) || (rev->n_slots > 0 && !c.d_angles_rev)) return QMLE_ERR_INVALID_ARG;
  // one operator per pass on LIVE states, in tape order
  for (const qmle_plan *p : {(const qmle_plan *)fwd, (const qmle_plan *)rev})
    if (!(p->flags & QMLE_PLAN_NO_FUSION) || (p->flags & QMLE_PLAN_INTERNAL_ZERO_RUN)) return QMLE_ERR_UNSUPPORTED;
  for (const qmle_plan *p : {(const qmle_plan *)fwd, (const qmle_plan *)rev}) {
    int last = -1;
    for (size_t k = 0; k < Unit::count(p); ++k) {
      const int op = Unit::src(p, k);
      if (op <= last) return QMLE_ERR_INVALID_ARG;
      last = op;
    }
  }
  ZMasks z = {};
  DensSeedTerms<T> seed = {};
  if (pauli) {
    const int rc = pauli_seed_check(ns, c.obs.obs_terms, c.obs.n_obs_terms, c.obs.n_obs);
    if (rc != QMLE_OK) return rc;
    if (c.obs.n_obs_terms > kDensMaxSeedTerms) return QMLE_ERR_UNSUPPORTED;
    seed.n = c.obs.n_obs_terms;
    for (int t = 0; t < seed.n; ++t) {
      seed.x[t] = wires_to_pos(c.obs.obs_terms[t].x_wires, ns);
      seed.z[t] = wires_to_pos(c.obs.obs_terms[t].z_wires, ns);
      seed.obs[t] = c.obs.obs_terms[t].obs;
      seed.coef[t] = (T)c.obs.obs_terms[t].coef;
    }
  } else {
    if (c.obs.n_obs > QMLE_MAX_QUBITS) return QMLE_ERR_INVALID_ARG;
    const int rc = zmasks_fill(c.obs.wire_masks, c.obs.n_obs, ns, z);
    if (rc != QMLE_OK) return rc;
  }
  for (int s = 0; s < c.n_steps; ++s) {
    const int rc = dens_check_step(c.steps[s], ns, (int)fwd->ops.size(), (int)rev->ops.size(), fwd->n_slots, c.n_chan,
                                   c.n_grad_slots);
    if (rc != QMLE_OK) return rc;
    if (s && c.steps[s].fwd_first <= c.steps[s - 1].fwd_first) return QMLE_ERR_INVALID_ARG;  // tape order
    if (s && c.steps[s].rev_first >= c.steps[s - 1].rev_first) return QMLE_ERR_INVALID_ARG;
  }
  DensWalk wf, wr;
  int rc = dens_walk(c.steps, c.n_steps, (int)fwd->ops.size(), false, wf);
  if (rc == QMLE_OK) rc = dens_walk(c.steps, c.n_steps, (int)rev->ops.size(), true, wr);
  if (rc != QMLE_OK) return rc;
  const DensLayout L = dens_layout<V, Unit>(fwd, rev, c.batch, c.n_cot, c.n_steps);
  char *ws = (char *)c.d_ws;
  size_t ws_bytes = c.ws_bytes;
  if (!align_workspace(ws, ws_bytes) || ws_bytes < L.total) return QMLE_ERR_WORKSPACE;

  // ---- device work from here on ----
  hipStream_t stream = (hipStream_t)c.stream;
  rc = Unit::ensure(fwd);
  if (rc == QMLE_OK) rc = Unit::ensure(rev);
  if (rc != QMLE_OK) return rc;
  T *fmats = (T *)(ws + L.fmats), *rmats = (T *)(ws + L.rmats);
  V *partial = (V *)(ws + L.partial), *ckpt = (V *)(ws + L.ckpt), *lam = (V *)(ws + L.lam);
  const size_t state = (size_t)1 << n, ck_stride = (size_t)c.batch * state;
  rc = Unit::build(fwd, c.d_angles_fwd, fmats, c.batch, stream);
  if (rc == QMLE_OK) rc = Unit::build(rev, c.d_angles_rev, rmats, rows, stream);
  if (rc != QMLE_OK) return rc;
  HIPCHK(hipMemsetAsync(c.d_grad, 0, (size_t)rows * c.n_grad_slots * sizeof(T), stream));
  const unsigned gx = grid_for(state, 256, 1u << 14);
  hipLaunchKernelGGL((k_dens_init<V>), dim3(gx, c.batch), dim3(256), 0, stream, ckpt, n);

  auto launch_step = [&](int s, bool backward) {
    const qmle_density_step &st = c.steps[s];
    const DensStepDev a = dens_step_dev(st, n, c.batch, fwd->n_slots);
    const T *chan = st.chan_off >= 0 ? c.d_chan + st.chan_off : nullptr;
    const V *src = ckpt + (size_t)s * ck_stride;
    if (!backward) {
      V *dst = ckpt + (size_t)(s + 1) * ck_stride;
      if (dens_step_bits(st) == 2) dens_launch_fwd<V, T, 2>(src, dst, c.d_angles_fwd, chan, a, stream);
      else dens_launch_fwd<V, T, 4>(src, dst, c.d_angles_fwd, chan, a, stream);
      return;
    }
    const int nbk = dens_blocks(n, dens_step_bits(st));
    if (dens_step_bits(st) == 2) dens_launch_bwd<V, T, 2>(src, lam, c.d_angles_fwd, chan, a, rows, partial, stream);
    else dens_launch_bwd<V, T, 4>(src, lam, c.d_angles_fwd, chan, a, rows, partial, stream);
    hipLaunchKernelGGL((k_adj_final<V, T>), dim3(rows), dim3(nbk >= 256 ? 256 : 64), 0, stream, (const V *)partial, nbk,
                       st.term.n_y, (T)st.term.coef, c.d_grad, c.n_grad_slots, st.term.out_slot);
  };

  // forward: term-free operators in place on the newest checkpoint, a step from checkpoint k to k + 1
  int newest = 0;
  for (size_t k = 0; k < Unit::count(fwd); ++k) {
    const int op = Unit::src(fwd, k);
    if (wf.step_of[op] >= 0) {
      if (wf.first_of[op] >= 0) {
        launch_step(wf.first_of[op], false);
        newest = wf.first_of[op] + 1;
      }
      continue;
    }
    rc = Unit::apply(fwd, k, ckpt + (size_t)newest * ck_stride, fmats, c.d_angles_fwd, c.batch, stream);
    if (rc != QMLE_OK) return rc;
  }
  // seed
  if (pauli) {
    HIPCHK(hipMemsetAsync(lam, 0, (size_t)rows * state * sizeof(V), stream));
    hipLaunchKernelGGL((k_dens_seed_pauli<V, T>), dim3(grid_for((uint64_t)1 << ns, 256, 1u << 14), rows), dim3(256), 0,
                       stream, lam, ns, c.d_weights, c.obs.n_obs, seed);
  } else {
    hipLaunchKernelGGL((k_dens_seed_z<V, T>), dim3(gx, rows), dim3(256), 0, stream, lam, ns, c.d_weights, z, c.obs.n_obs);
  }
  // backward: the daggered term-free operators on lambda alone, a step against its checkpoint
  int left = c.n_steps;
  for (size_t k = 0; k < Unit::count(rev) && left > 0; ++k) {
    const int op = Unit::src(rev, k);
    if (wr.step_of[op] >= 0) {
      if (wr.first_of[op] >= 0) {
        launch_step(wr.first_of[op], true);
        --left;
      }
      continue;
    }
    rc = Unit::apply(rev, k, lam, rmats, c.d_angles_rev, rows, stream);
    if (rc != QMLE_OK) return rc;
  }
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

}  // namespace
