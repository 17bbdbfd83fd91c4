// Hamiltonian time evolution: U(t1) of dU/dt = -i sum_i f_i(t) H_i U for 2x2 and 4x4 U, one solve per row, on the
// fixed grid of the reference's commutator-free Magnus integrators (qml_essentials/evolution.py:204-231):
//   order 2  U <- exp(h A(t_n + h / 2)) U                                                  one node per step
//   order 4  U <- exp(Omega_b) exp(Omega_a) U,  Omega_a = h (a1 A1 + a2 A2), Omega_b = h (a2 A1 + a1 A2),
//            A_k = A(t_n + c_k h), c_1,2 = 1/2 -+ sqrt(3)/6, a_1,2 = 1/4 +- sqrt(3)/6       two nodes per step
// with A(t) = -i sum_i c_i(t) H_i.  The kernel evaluates no coefficient function: it reads c_i at the node times from
// a table coef[row][node][term], in node order.  float64 throughout; the result is rounded once when it is stored as
// complex64.
//
// Work split.  A row's steps are cut into `lanes` contiguous runs (1, 4, 16 or 64 neighbouring lanes of one wave).
// Every lane forms the ordered product of its run from the identity; the partial products are then multiplied in
// time order (later run on the left) in log2(lanes) rounds of lane shifts inside the wave -- neither LDS nor HBM.
// Matrix multiplication is associative, so the split changes the result through rounding only.
//
// Registers (DIM is a template parameter; every matrix index is a compile-time constant, nothing is indexed at run
// time, no scratch).  DIM = 2: U is 8 doubles, exp in closed form.  DIM = 4: U is 32 doubles (64 VGPRs).  h sum c_i H_i
// is Hermitian and is kept packed -- 4 real diagonal entries and the 6 complex entries above it, 16 doubles -- and
// exp(Omega) is never formed: exp(Omega) U acts on the columns of U independently, so each column takes its own
// Taylor series v + Omega v + Omega (Omega v) / 2 + ..., which needs the column (8 doubles), the running term (8) and
// one product (8) beside U and the packed matrix: about 64 + 32 + 48 VGPRs and their temporaries.  The combine step
// holds the partner's 32 doubles beside its own and overwrites its own column by column.
//
// The series.  With nu = the largest absolute row sum of h sum c_i H_i (a bound of the 2-norm), the exponent is cut into
// m = ceil(nu / 0.5) equal parts (m = 1 on any grid that resolves the pulse) and each part's series runs until the
// bound (nu / m)^k / k! of the next term falls below 1e-19, at most 24 terms: the count follows from the norm, decided
// before the first product, never from the iterates.  Rows whose nu is not finite or exceeds 2^15 come back as NaN.
#include "qmle_host.h"
#include "qmle_dev.h"

namespace {

constexpr int kEvolveMaxTerms = 16;     // Hermitian terms per call (they travel as kernel arguments)
constexpr int kEvolveThreads = 256;
constexpr double kEvolveTheta = 0.5;    // norm of one part of the exponent
constexpr double kEvolveMaxNorm = 32768.0;

// the terms, packed per term as DIM real diagonal entries, then the real and the imaginary parts of the DIM (DIM - 1) / 2
// entries above the diagonal in row-major order -- DIM * DIM doubles
struct EvolveTerms {
  double h[kEvolveMaxTerms][16];
};

template <int DIM> struct Herm {
  static constexpr int NU = DIM * (DIM - 1) / 2;
  double d[DIM], re[NU], im[NU];
};
// index of entry (i, j), i < j, among the entries above the diagonal
template <int DIM> __host__ __device__ constexpr int upper_index(int i, int j) { return i * (2 * DIM - i - 1) / 2 + (j - i - 1); }

template <int DIM> struct CMat {
  double re[DIM * DIM], im[DIM * DIM];  // row-major
};

template <int DIM> __host__ __device__ __forceinline__ void set_identity(CMat<DIM> &U) {
#pragma unroll
  for (int i = 0; i < DIM * DIM; ++i) {
    U.re[i] = (i / DIM == i % DIM) ? 1.0 : 0.0;
    U.im[i] = 0.0;
  }
}

// G = sum_i w_i H_i for the weights w (already times h)
template <int DIM>
__host__ __device__ __forceinline__ void weighted_sum(const EvolveTerms &T, int n_terms, const double *__restrict__ c0,
                                             const double *__restrict__ c1, double w0, double w1, Herm<DIM> &G) {
#pragma unroll
  for (int k = 0; k < DIM; ++k) G.d[k] = 0.0;
#pragma unroll
  for (int k = 0; k < Herm<DIM>::NU; ++k) G.re[k] = G.im[k] = 0.0;
  for (int t = 0; t < n_terms; ++t) {
    double w = w0 * c0[t];
    if (c1) w = fma(w1, c1[t], w);
    const double *__restrict__ H = T.h[t];
#pragma unroll
    for (int k = 0; k < DIM; ++k) G.d[k] = fma(w, H[k], G.d[k]);
#pragma unroll
    for (int k = 0; k < Herm<DIM>::NU; ++k) {
      G.re[k] = fma(w, H[DIM + k], G.re[k]);
      G.im[k] = fma(w, H[DIM + Herm<DIM>::NU + k], G.im[k]);
    }
  }
}

// U <- exp(-i G) U, G = g0 I + a . sigma:  exp(-i G) = e^{-i g0} (cos |a| I - i sin |a| / |a| (a . sigma))
__host__ __device__ __forceinline__ void apply_exp(const Herm<2> &G, CMat<2> &U) {
  const double g0 = 0.5 * (G.d[0] + G.d[1]), az = 0.5 * (G.d[0] - G.d[1]), ax = G.re[0], ay = -G.im[0];
  const double r = sqrt(ax * ax + ay * ay + az * az);
  double s, c, ps, pc;
  sincos(r, &s, &c);
  const double sinc = r < 1e-4 ? 1.0 - r * r * (1.0 / 6.0) * (1.0 - r * r * 0.05) : s / r;  // |a| -> 0: the series
  sincos(g0, &ps, &pc);
  // E = (pc - i ps) * [[c - i sinc az, -i sinc (ax - i ay)], [-i sinc (ax + i ay), c + i sinc az]]
  const double m_re[4] = {c, -sinc * ay, sinc * ay, c}, m_im[4] = {-sinc * az, -sinc * ax, -sinc * ax, sinc * az};
  double e_re[4], e_im[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e_re[k] = pc * m_re[k] + ps * m_im[k];
    e_im[k] = pc * m_im[k] - ps * m_re[k];
  }
  CMat<2> R;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      double xr = 0.0, xi = 0.0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        xr = fma(e_re[2 * i + k], U.re[2 * k + j], xr);
        xr = fma(-e_im[2 * i + k], U.im[2 * k + j], xr);
        xi = fma(e_re[2 * i + k], U.im[2 * k + j], xi);
        xi = fma(e_im[2 * i + k], U.re[2 * k + j], xi);
      }
      R.re[2 * i + j] = xr;
      R.im[2 * i + j] = xi;
    }
  U = R;
}

// y = G v for the packed Hermitian G and one complex column v
__host__ __device__ __forceinline__ void herm_matvec(const Herm<4> &G, const double (&vr)[4], const double (&vi)[4],
                                            double (&yr)[4], double (&yi)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double xr = G.d[i] * vr[i], xi = G.d[i] * vi[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j == i) continue;
      const int u = j > i ? upper_index<4>(i, j) : upper_index<4>(j, i);
      const double gr = G.re[u], gi = j > i ? G.im[u] : -G.im[u];  // below the diagonal: the conjugate
      xr = fma(gr, vr[j], xr);
      xr = fma(-gi, vi[j], xr);
      xi = fma(gr, vi[j], xi);
      xi = fma(gi, vr[j], xi);
    }
    yr[i] = xr;
    yi[i] = xi;
  }
}

// U <- exp(-i G) U, column by column (see the head of this file)
__host__ __device__ __forceinline__ void apply_exp(const Herm<4> &G, CMat<4> &U) {
  double nu = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double row = fabs(G.d[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j == i) continue;
      const int u = j > i ? upper_index<4>(i, j) : upper_index<4>(j, i);
      row += fabs(G.re[u]) + fabs(G.im[u]);
    }
    nu = fmax(nu, row);
  }
  if (!(nu <= kEvolveMaxNorm)) {  // (also a NaN)
    const double bad = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 16; ++k) U.re[k] = U.im[k] = bad;
    return;
  }
  const int parts = nu > kEvolveTheta ? (int)ceil(nu / kEvolveTheta) : 1;
  const double inv_parts = 1.0 / (double)parts, nu_part = nu * inv_parts;
  int n_series = 1;  // terms behind the column itself
  for (double bound = nu_part; n_series < 24 && bound >= 1e-19; ++n_series) bound *= nu_part / (double)(n_series + 1);
#pragma unroll
  for (int col = 0; col < 4; ++col) {
    double vr[4], vi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vr[i] = U.re[4 * i + col];
      vi[i] = U.im[4 * i + col];
    }
    for (int p = 0; p < parts; ++p) {
      double tr[4], ti[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        tr[i] = vr[i];
        ti[i] = vi[i];
      }
      for (int k = 1; k <= n_series; ++k) {
        double yr[4], yi[4];
        herm_matvec(G, tr, ti, yr, yi);
        const double f = inv_parts / (double)k;  // term <- (-i G / parts) term / k
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          tr[i] = f * yi[i];
          ti[i] = -f * yr[i];
          vr[i] += tr[i];
          vi[i] += ti[i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      U.re[4 * i + col] = vr[i];
      U.im[4 * i + col] = vi[i];
    }
  }
}

// P <- L P, one column of P at a time
template <int DIM> __host__ __device__ __forceinline__ void multiply_left(const CMat<DIM> &L, CMat<DIM> &P) {
#pragma unroll
  for (int j = 0; j < DIM; ++j) {
    double cr[DIM], ci[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      double xr = 0.0, xi = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        xr = fma(L.re[DIM * i + k], P.re[DIM * k + j], xr);
        xr = fma(-L.im[DIM * i + k], P.im[DIM * k + j], xr);
        xi = fma(L.re[DIM * i + k], P.im[DIM * k + j], xi);
        xi = fma(L.im[DIM * i + k], P.re[DIM * k + j], xi);
      }
      cr[i] = xr;
      ci[i] = xi;
    }
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      P.re[DIM * i + j] = cr[i];
      P.im[DIM * i + j] = ci[i];
    }
  }
}
// P <- L P for the later partial product L held `delta` lanes up (lanes: the row's lanes, a power of two <= 64)
template <int DIM> __device__ __forceinline__ void combine_with_later(CMat<DIM> &P, int delta, int lanes) {
  CMat<DIM> L;
#pragma unroll
  for (int k = 0; k < DIM * DIM; ++k) {
    L.re[k] = __shfl_down(P.re[k], delta, lanes);
    L.im[k] = __shfl_down(P.im[k], delta, lanes);
  }
  multiply_left(L, P);
}

// One work item per (row, lane of the row); a block holds kEvolveThreads / lanes rows.
template <int DIM, int ORDER>
__global__ __launch_bounds__(kEvolveThreads) void k_evolve_magnus(const EvolveTerms terms, int n_terms,
                                                                  const double *__restrict__ coef,
                                                                  const double *__restrict__ h_rows, int rows,
                                                                  int n_steps, int lanes, int out_f64,
                                                                  void *__restrict__ out) {
  const long long gid = (long long)blockIdx.x * kEvolveThreads + threadIdx.x;
  const long long row_ll = gid / lanes;
  const int lane = (int)(gid - row_ll * lanes);
  const bool live = row_ll < rows;  // (a row's lanes are live or idle together: lanes divides the block)
  const int row = live ? (int)row_ll : rows - 1;
  const int s_begin = (int)((long long)lane * n_steps / lanes), s_end = (int)((long long)(lane + 1) * n_steps / lanes);
  constexpr int NODES = ORDER == 4 ? 2 : 1;
  const double h = h_rows[row];
  const double *__restrict__ c = coef + ((size_t)row * n_steps * NODES + (size_t)s_begin * NODES) * n_terms;
  constexpr double kA1 = 0.25 + 0.28867513459481288225, kA2 = 0.25 - 0.28867513459481288225;  // 1/4 +- sqrt(3)/6
  CMat<DIM> U;
  set_identity(U);
  Herm<DIM> G;
  for (int s = s_begin; s < s_end; ++s, c += (size_t)NODES * n_terms) {
    if constexpr (ORDER == 2) {
      weighted_sum<DIM>(terms, n_terms, c, nullptr, h, 0.0, G);
      apply_exp(G, U);
    } else {
      weighted_sum<DIM>(terms, n_terms, c, c + n_terms, h * kA1, h * kA2, G);  // Omega_a first
      apply_exp(G, U);
      weighted_sum<DIM>(terms, n_terms, c, c + n_terms, h * kA2, h * kA1, G);  // then Omega_b
      apply_exp(G, U);
    }
  }
  for (int delta = 1; delta < lanes; delta <<= 1) combine_with_later(U, delta, lanes);  // lane 0 ends with the row
  if (!live || lane != 0) return;
  if (out_f64) {
    double2 *o = (double2 *)out + (size_t)row * (DIM * DIM);
#pragma unroll
    for (int k = 0; k < DIM * DIM; ++k) o[k] = make_double2(U.re[k], U.im[k]);
  } else {
    float2 *o = (float2 *)out + (size_t)row * (DIM * DIM);
#pragma unroll
    for (int k = 0; k < DIM * DIM; ++k) o[k] = make_float2((float)U.re[k], (float)U.im[k]);
  }
}

// lanes_per_row = 0: one lane per row when the rows alone fill the card (256 CUs x 4 SIMDs x 2 waves), else the
// widest split that stays within that many lanes and leaves every lane at least one step
int evolve_auto_lanes(int rows, int n_steps) {
  const long long fill = 256ll * 4 * 2 * kWave;
  int lanes = 1;
  for (int cand : {4, 16, 64})
    if ((long long)rows * cand <= fill && cand <= n_steps) lanes = cand;
  return lanes;
}

template <int DIM> void pack_terms(const double *h_terms, int n_terms, EvolveTerms &T) {
  for (int t = 0; t < n_terms; ++t) {
    const double *H = h_terms + (size_t)t * DIM * DIM * 2;  // complex128, row-major
    for (int k = 0; k < 16; ++k) T.h[t][k] = 0.0;
    for (int i = 0; i < DIM; ++i) {
      T.h[t][i] = H[2 * (i * DIM + i)];
      for (int j = i + 1; j < DIM; ++j) {
        const int u = upper_index<DIM>(i, j);
        T.h[t][DIM + u] = H[2 * (i * DIM + j)];
        T.h[t][DIM + DIM * (DIM - 1) / 2 + u] = H[2 * (i * DIM + j) + 1];
      }
    }
  }
}

}  // namespace

extern "C" {

int qmle_evolve_lanes(int rows, int n_steps) {
  if (rows < 1 || n_steps < 1) return QMLE_ERR_INVALID_ARG;
  return evolve_auto_lanes(rows, n_steps);
}

int qmle_evolve_magnus(const double *h_terms, int n_terms, int dim, const double *d_coef, const double *d_h, int rows,
                       int order, int n_steps, int lanes_per_row, int out_f64, void *d_out, qmle_stream stream_) {
  if (dim != 2 && dim != 4) return QMLE_ERR_UNSUPPORTED;
  if (order != 2 && order != 4) return QMLE_ERR_UNSUPPORTED;
  if (!h_terms || !d_coef || !d_h || !d_out || n_terms < 1 || n_terms > kEvolveMaxTerms || rows < 1 || n_steps < 1 ||
      (out_f64 != 0 && out_f64 != 1))
    return QMLE_ERR_INVALID_ARG;
  if (lanes_per_row != 0 && lanes_per_row != 1 && lanes_per_row != 4 && lanes_per_row != 16 && lanes_per_row != 64)
    return QMLE_ERR_INVALID_ARG;
  if ((long long)n_steps * (order == 4 ? 2 : 1) * n_terms > (1ll << 31) - 1) return QMLE_ERR_INVALID_ARG;
  const int lanes = lanes_per_row ? lanes_per_row : evolve_auto_lanes(rows, n_steps);
  const long long items = (long long)rows * lanes;
  if (items > (1ll << 31) - kEvolveThreads) return QMLE_ERR_INVALID_ARG;  // grid.x
  EvolveTerms T;
  if (dim == 2) pack_terms<2>(h_terms, n_terms, T);
  else pack_terms<4>(h_terms, n_terms, T);
  for (int t = n_terms; t < kEvolveMaxTerms; ++t)
    for (int k = 0; k < 16; ++k) T.h[t][k] = 0.0;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(grid_for((uint64_t)items, kEvolveThreads)), block(kEvolveThreads);
#define QMLE_EVOLVE_LAUNCH(D, O)                                                                                  \
  hipLaunchKernelGGL((k_evolve_magnus<D, O>), grid, block, 0, stream, T, n_terms, d_coef, d_h, rows, n_steps, lanes, \
                     out_f64, d_out)
  if (dim == 2 && order == 2) QMLE_EVOLVE_LAUNCH(2, 2);
  else if (dim == 2) QMLE_EVOLVE_LAUNCH(2, 4);
  else if (order == 2) QMLE_EVOLVE_LAUNCH(4, 2);
  else QMLE_EVOLVE_LAUNCH(4, 4);
#undef QMLE_EVOLVE_LAUNCH
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

}  // extern "C"
