// Hamiltonian time evolution: U(t1) of dU/dt = -i sum_i f_i(t) H_i U for 2x2 and 4x4 U, one solve per row, on the
// fixed grid of the reference's commutator-free Magnus integrators (qml_essentials/evolution.py:204-231):
//   order 2  U <- exp(h A(t_n + h / 2)) U                                                  one node per step
//   order 4  U <- exp(Omega_b) exp(Omega_a) U,  Omega_a = h (a1 A1 + a2 A2), Omega_b = h (a2 A1 + a1 A2),
//            A_k = A(t_n + c_k h), c_1,2 = 1/2 -+ sqrt(3)/6, a_1,2 = 1/4 +- sqrt(3)/6       two nodes per step
// with A(t) = -i sum_i c_i(t) H_i.  The kernel evaluates no coefficient function: it reads c_i at the node times from
// a table coef[row][node][term], in node order.  float64 throughout; the result is rounded once when it is stored as
// complex64.  k_pulse_unitaries (further down) solves the RX / RY leaves of pulse-level gates on the same grids with
// the same work split, but evaluates its two coefficients itself instead of reading a table; k_pulse_jac adds its
// parameter sensitivities and k_evolve_magnus_jac the directional derivatives of the table-driven solve (their own
// comment blocks).  k_compose_circuits (last)
// multiplies such 2x2 results and constant gates into the unitaries of 1- and 2-wire circuits with their parameter
// derivatives: its own comment block.
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
#include <algorithm>
#include <type_traits>
#include <vector>

#include "qmle_host.h"
#include "qmle_dev.h"

namespace {

constexpr int kEvolveMaxTerms = 16;     // Hermitian terms per call (they travel as kernel arguments)
constexpr int kEvolveThreads = 256;
constexpr double kEvolveTheta = 0.5;    // norm of one part of the exponent
constexpr double kEvolveMaxNorm = 32768.0;
// the two Gauss-Legendre nodes of an order-4 step and their weights in Omega_a (Omega_b: exchanged)
constexpr double kC1 = 0.5 - 0.28867513459481288225, kC2 = 0.5 + 0.28867513459481288225;    // 1/2 -+ sqrt(3)/6
constexpr double kA1 = 0.25 + 0.28867513459481288225, kA2 = 0.25 - 0.28867513459481288225;  // 1/4 +- sqrt(3)/6

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

template <int DIM> __host__ __device__ __forceinline__ void set_zero(Herm<DIM> &G) {
#pragma unroll
  for (int k = 0; k < DIM; ++k) G.d[k] = 0.0;
#pragma unroll
  for (int k = 0; k < Herm<DIM>::NU; ++k) G.re[k] = G.im[k] = 0.0;
}
// G += sum_i w_i H_i for the weights w (already times h)
template <int DIM>
__host__ __device__ __forceinline__ void weighted_add(const EvolveTerms &T, int n_terms, const double *__restrict__ c0,
                                             const double *__restrict__ c1, double w0, double w1, Herm<DIM> &G) {
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
// G = sum_i w_i H_i
template <int DIM>
__host__ __device__ __forceinline__ void weighted_sum(const EvolveTerms &T, int n_terms, const double *__restrict__ c0,
                                             const double *__restrict__ c1, double w0, double w1, Herm<DIM> &G) {
  set_zero(G);
  weighted_add<DIM>(T, n_terms, c0, c1, w0, w1, G);
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

// y = G v (ACC: y += G v) for the packed Hermitian G and one complex column v
template <bool ACC = false>
__host__ __device__ __forceinline__ void herm_matvec(const Herm<4> &G, const double (&vr)[4], const double (&vi)[4],
                                            double (&yr)[4], double (&yi)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double xr = ACC ? fma(G.d[i], vr[i], yr[i]) : G.d[i] * vr[i], xi = ACC ? fma(G.d[i], vi[i], yi[i]) : G.d[i] * vi[i];
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

// the largest absolute row sum of a packed Hermitian matrix
__host__ __device__ __forceinline__ double herm_row_norm(const Herm<4> &G) {
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
    nu = (row > nu || row != row) ? row : nu;  // (a NaN stays)
  }
  return nu;
}
// How the series of exp(-i G) runs, from the norm alone (the head of this file): the forward kernel and the Jacobian
// kernel take it from here, so slot 0 of the latter repeats the former bit for bit.
struct SeriesCut {
  bool ok;            // the norm is finite and within kEvolveMaxNorm
  int parts;          // equal parts the exponent is cut into
  double inv_parts;
  int n_series;       // terms behind the column itself
};
__host__ __device__ __forceinline__ SeriesCut series_cut_norm(double nu) {
  SeriesCut c;
  c.ok = nu <= kEvolveMaxNorm;  // (false for a NaN)
  c.parts = c.ok && nu > kEvolveTheta ? (int)ceil(nu / kEvolveTheta) : 1;
  c.inv_parts = 1.0 / (double)c.parts;
  const double nu_part = nu * c.inv_parts;
  c.n_series = 1;
  for (double bound = nu_part; c.n_series < 24 && bound >= 1e-19; ++c.n_series) bound *= nu_part / (double)(c.n_series + 1);
  return c;
}
__host__ __device__ __forceinline__ SeriesCut series_cut(const Herm<4> &G) { return series_cut_norm(herm_row_norm(G)); }

// U <- exp(-i G) U, column by column (see the head of this file)
__host__ __device__ __forceinline__ void apply_exp(const Herm<4> &G, CMat<4> &U) {
  const SeriesCut cut = series_cut(G);
  if (!cut.ok) {
    const double bad = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 16; ++k) U.re[k] = U.im[k] = bad;
    return;
  }
  const int parts = cut.parts, n_series = cut.n_series;
  const double inv_parts = cut.inv_parts;
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

// ---- pulse-level gates: every RX / RY pulse solve of a tape in one launch -------------------------------------------
// One solve per (request, row): d_solves[solve] = {p0, p1, p2, w, T, axis, -, -}.  The Hamiltonian is
// cx(t) X + cy(t) Y with the reference's interaction-picture coefficients (qml_essentials/pulses.py:446-630), which the
// lanes evaluate at their own node times in float64 -- no coefficient table.  The envelope centre is t_c = t / 2 with t
// the RUNNING time (the reference's definition, which its optimised defaults assume), so
//   gaussian  A exp(-(t / 2 sigma)^2 / 2)          p = {A, sigma}
//   square    A for t <= width, else 0             p = {A, width}
//   cosine    A cos(pi clip(t / (2 width), +-1/2)) p = {A, width}
//   drag      g (1 - beta (t / 2) / sigma^2), g the gaussian   p = {A, beta, sigma}
//   sech      A / cosh(t / 2 sigma)                p = {A, sigma}
// Node times are absolute (the carrier phase depends on t).  The grid covers the envelope's support: [0, min(T, width)]
// for square and cosine, whose coefficient is identically zero beyond it -- a grid over [0, T] would straddle the jump
// (square) or the kink (cosine) and lose the order of the scheme -- and [0, T] otherwise.
enum { kEnvGaussian = 0, kEnvSquare = 1, kEnvCosine = 2, kEnvDrag = 3, kEnvSech = 4, kEnvCount = 5 };
enum { kModeRwa = 0, kModeLab = 1, kModeDrive = 2, kModeCount = 3 };
constexpr double kPi = 3.14159265358979323846;

struct PulseLaunch {
  int envelope, mode, n_solves, n_steps, lanes, out_f64;
  double omega_c, omega_q;
};

template <int ENV>
__host__ __device__ __forceinline__ double pulse_envelope(double p0, double p1, double p2, double t) {
  const double tc = 0.5 * t;  // t - t_c
  if constexpr (ENV == kEnvGaussian) {
    const double x = tc / p1;
    return p0 * exp(-0.5 * (x * x));
  } else if constexpr (ENV == kEnvSquare) {
    return fabs(tc) <= 0.5 * p1 ? p0 : 0.0;
  } else if constexpr (ENV == kEnvCosine) {
    const double x = fmin(fmax(tc / p1, -0.5), 0.5);
    return p0 * cos(kPi * x);
  } else if constexpr (ENV == kEnvDrag) {
    const double x = tc / p2, g = p0 * exp(-0.5 * (x * x));
    return g + p1 * (g * (-tc / (p2 * p2)));
  } else {
    const double e = exp(-fabs(tc / p1));  // 1 / cosh x = 2 e^-|x| / (1 + e^-2|x|): one exponential, no overflow
    return p0 * (2.0 * e / fma(e, e, 1.0));
  }
}

// sin and cos of two arguments through ONE copy of the fp64 argument reduction (the loop stays rolled: the
// transcendental code and its constants are what fills the scalar registers of these kernels)
__host__ __device__ __forceinline__ void sincos_pair(double a0, double a1, double &s0, double &c0, double &s1, double &c1) {
  s0 = c0 = s1 = c1 = 0.0;
#pragma nounroll
  for (int k = 0; k < 2; ++k) {
    double sn, cs;
    sincos(k ? a1 : a0, &sn, &cs);
    if (k) s1 = sn, c1 = cs;
    else s0 = sn, c0 = cs;
  }
}

// the X and Y coefficients at time t; axis_y: the RY pulse (carrier phase +pi/2)
template <int ENV, int MODE>
__host__ __device__ __forceinline__ void pulse_coefficients(const PulseLaunch &L, double p0, double p1, double p2, double w,
                                                   bool axis_y, double t, double &cx, double &cy) {
#pragma clang fp contract(off)  // omega t + phi reaches 160 rad: a fused multiply-add would move the phase by an ulp of it
  const double env = pulse_envelope<ENV>(p0, p1, p2, t);
  if constexpr (MODE == kModeRwa) {
    const double c = 0.5 * env * w;
    cx = axis_y ? 0.0 : c;
    cy = axis_y ? c : 0.0;
  } else if constexpr (MODE == kModeLab) {
    double sq, cq, sc, carrier;
    sincos_pair(L.omega_q * t, L.omega_c * t + (axis_y ? 0.5 * kPi : 0.0), sq, cq, sc, carrier);
    cx = env * carrier * cq * w;
    cy = -env * carrier * sq * w;
  } else {  // product-to-sum form of the same coefficients
    double sd, cd, ss, cs;
    sincos_pair((L.omega_c - L.omega_q) * t, (L.omega_c + L.omega_q) * t, sd, cd, ss, cs);
    const double mx = axis_y ? -0.5 * (ss + sd) : 0.5 * (cd + cs);
    const double my = axis_y ? -0.5 * (cs - cd) : -0.5 * (ss - sd);
    cx = env * mx * w;
    cy = env * my * w;
  }
}

// U <- exp(-i (gx X + gy Y)) U; false when the exponent's norm is not finite or beyond kEvolveMaxNorm
__host__ __device__ __forceinline__ bool pulse_step(double gx, double gy, CMat<2> &U) {
  Herm<2> G;
  G.d[0] = G.d[1] = 0.0;
  G.re[0] = gx;
  G.im[0] = -gy;
  apply_exp(G, U);
  return fabs(gx) + fabs(gy) <= kEvolveMaxNorm;
}

// what a work item of the pulse kernels is: its solve's row, its lane of the solve and that lane's run of steps
struct PulseItem {
  double p0, p1, p2, w, T;
  bool axis_y, live;  // (a solve's lanes are live or idle together: lanes divides the block)
  int solve, lane, s_begin, s_end;
};
__device__ __forceinline__ PulseItem pulse_item(const double *__restrict__ solves, const PulseLaunch &L) {
  const long long gid = (long long)blockIdx.x * kEvolveThreads + threadIdx.x;
  const long long solve_ll = gid / L.lanes;
  PulseItem I;
  I.lane = (int)(gid - solve_ll * L.lanes);
  I.live = solve_ll < L.n_solves;
  I.solve = I.live ? (int)solve_ll : L.n_solves - 1;
  const double *__restrict__ q = solves + (size_t)I.solve * 8;
  I.p0 = q[0], I.p1 = q[1], I.p2 = q[2], I.w = q[3], I.T = q[4], I.axis_y = q[5] != 0.0;
  I.s_begin = (int)((long long)I.lane * L.n_steps / L.lanes);
  I.s_end = (int)((long long)(I.lane + 1) * L.n_steps / L.lanes);
  return I;
}

// One work item per (solve, lane of the solve); a block holds kEvolveThreads / lanes solves.
template <int ORDER, int ENV, int MODE>
__global__ __launch_bounds__(kEvolveThreads) void k_pulse_unitaries(const double *__restrict__ solves, const PulseLaunch L,
                                                                    void *__restrict__ out,
                                                                    const void *__restrict__ prev,
                                                                    double *__restrict__ err) {
  const int lanes = L.lanes, n_steps = L.n_steps;
  const auto [p0, p1, p2, w, T, axis_y, live, solve, lane, s_begin, s_end] = pulse_item(solves, L);
  const double span = (ENV == kEnvSquare || ENV == kEnvCosine) ? fmin(T, p1) : T;
  const double h = span / (double)n_steps;
  CMat<2> U;
  set_identity(U);
  bool ok = true;
  for (int s = s_begin; s < s_end; ++s) {
    double ax, ay;
    if constexpr (ORDER == 2) {
      pulse_coefficients<ENV, MODE>(L, p0, p1, p2, w, axis_y, ((double)s + 0.5) * h, ax, ay);
      ok &= pulse_step(h * ax, h * ay, U);
    } else {
      double bx = 0.0, by = 0.0;
      ax = ay = 0.0;
#pragma nounroll  // (one copy of the transcendental code serves both nodes)
      for (int node = 0; node < 2; ++node) {
        double x, y;
        pulse_coefficients<ENV, MODE>(L, p0, p1, p2, w, axis_y, ((double)s + (node ? kC2 : kC1)) * h, x, y);
        if (node) bx = x, by = y;
        else ax = x, ay = y;
      }
      const double h1 = h * kA1, h2 = h * kA2;
#pragma nounroll
      for (int half = 0; half < 2; ++half) {  // Omega_a first, then Omega_b
        const double wa = half ? h2 : h1, wb = half ? h1 : h2;
        ok &= pulse_step(fma(wb, bx, wa * ax), fma(wb, by, wa * ay), U);
      }
    }
  }
  if (!ok) {  // (the combine carries the NaN into lane 0)
    const double bad = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 4; ++k) U.re[k] = U.im[k] = bad;
  }
  for (int delta = 1; delta < lanes; delta <<= 1) combine_with_later(U, delta, lanes);  // lane 0 ends with the solve
  if (!live || lane != 0) return;
  double worst = 0.0;  // max |U - U_prev|; NaN once an entry is NaN
  if (L.out_f64) {
    double2 *o = (double2 *)out + (size_t)solve * 4;
    const double2 *pv = prev ? (const double2 *)prev + (size_t)solve * 4 : nullptr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (pv) {
        const double dr = U.re[k] - pv[k].x, di = U.im[k] - pv[k].y, a = sqrt(dr * dr + di * di);
        worst = (a > worst || a != a) ? a : worst;
      }
      o[k] = make_double2(U.re[k], U.im[k]);
    }
  } else {
    float2 *o = (float2 *)out + (size_t)solve * 4;
    const float2 *pv = prev ? (const float2 *)prev + (size_t)solve * 4 : nullptr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (pv) {
        const double dr = U.re[k] - (double)pv[k].x, di = U.im[k] - (double)pv[k].y, a = sqrt(dr * dr + di * di);
        worst = (a > worst || a != a) ? a : worst;
      }
      o[k] = make_float2((float)U.re[k], (float)U.im[k]);
    }
  }
  if (err) err[solve] = worst;
}

// ---- pulse solves with parameter sensitivities ------------------------------------------------------------------------
// The same solves with the exact derivative of the grid's result by the five arguments theta = p0, p1, p2, w, T
// (include/qmle_sv.h has the conventions).  A step's exponent is g = h sum_j a_j c(t_j), t_j = (s + c_j) h, so
//   dg/dtheta_k = h sum_j a_j dc/dtheta_k (t_j) + dh/dtheta_k sum_j a_j (c(t_j) + t_j dc/dt (t_j)),
// the second sum -- step length and moving nodes -- for T, or for the width of a square / cosine pulse that ends
// inside T.  Every lane carries (P, dP_1..5), 48 doubles, for its run of steps.
constexpr int kJacSlots = 6;  // U and its five derivatives

// e = {env, d env / d p0, d env / d p1, d env / d p2, d env / dt} at time t
template <int ENV>
__host__ __device__ __forceinline__ void pulse_envelope_jac(double p0, double p1, double p2, double t, double (&e)[5]) {
  const double tc = 0.5 * t;  // t - t_c, d tc / dt = 1 / 2
  e[3] = 0.0;
  if constexpr (ENV == kEnvGaussian) {
    const double x = tc / p1, f = exp(-0.5 * (x * x)), g = p0 * f;
    e[0] = g;
    e[1] = f;
    e[2] = g * (x * x) / p1;
    e[4] = -0.5 * g * x / p1;
  } else if constexpr (ENV == kEnvSquare) {
    const double on = fabs(tc) <= 0.5 * p1 ? 1.0 : 0.0;
    e[0] = p0 * on;
    e[1] = on;
    e[2] = e[4] = 0.0;  // piecewise constant: the derivative almost everywhere
  } else if constexpr (ENV == kEnvCosine) {
    const double x = tc / p1;
    double sn, cs;
    sincos(kPi * fmin(fmax(x, -0.5), 0.5), &sn, &cs);
    const double dx = fabs(x) <= 0.5 ? -kPi * p0 * sn : 0.0;  // d env / dx; the clipped part is flat
    e[0] = p0 * cs;
    e[1] = cs;
    e[2] = dx * (-x / p1);
    e[4] = dx * (0.5 / p1);
  } else if constexpr (ENV == kEnvDrag) {
    const double x = tc / p2, f = exp(-0.5 * (x * x)), g = p0 * f, u = tc / (p2 * p2), k = 1.0 - p1 * u;
    e[0] = g + p1 * (g * (-u));
    e[1] = f * k;
    e[2] = -g * u;
    e[3] = g * (x * x) / p2 * k + 2.0 * g * p1 * u / p2;
    e[4] = 0.5 * (-g * u * k - g * p1 / (p2 * p2));
  } else {
    const double u = tc / p1, ex = exp(-fabs(u)), den = fma(ex, ex, 1.0), sech = 2.0 * ex / den;
    const double th = copysign((1.0 - ex * ex) / den, u);  // tanh u
    e[0] = p0 * sech;
    e[1] = sech;
    e[2] = p0 * sech * th * u / p1;
    e[4] = -0.5 * p0 * sech * th / p1;
  }
}

// the carrier factors (kx, ky) of the X and Y coefficients, c = env k w, and their time derivatives
template <int MODE>
__host__ __device__ __forceinline__ void pulse_carrier_jac(const PulseLaunch &L, bool axis_y, double t, double (&k)[2],
                                                  double (&kt)[2]) {
#pragma clang fp contract(off)  // (as in pulse_coefficients)
  if constexpr (MODE == kModeRwa) {
    k[0] = axis_y ? 0.0 : 0.5;
    k[1] = axis_y ? 0.5 : 0.0;
    kt[0] = kt[1] = 0.0;
  } else if constexpr (MODE == kModeLab) {
    double sq, cq, sc, cc;
    sincos_pair(L.omega_q * t, L.omega_c * t + (axis_y ? 0.5 * kPi : 0.0), sq, cq, sc, cc);
    k[0] = cc * cq;
    k[1] = -cc * sq;
    kt[0] = -L.omega_c * sc * cq - L.omega_q * cc * sq;
    kt[1] = L.omega_c * sc * sq - L.omega_q * cc * cq;
  } else {
    const double od = L.omega_c - L.omega_q, os = L.omega_c + L.omega_q;
    double sd, cd, ss, cs;
    sincos_pair(od * t, os * t, sd, cd, ss, cs);
    k[0] = axis_y ? -0.5 * (ss + sd) : 0.5 * (cd + cs);
    k[1] = axis_y ? -0.5 * (cs - cd) : -0.5 * (ss - sd);
    kt[0] = axis_y ? -0.5 * (os * cs + od * cd) : -0.5 * (od * sd + os * ss);
    kt[1] = axis_y ? 0.5 * (os * ss - od * sd) : -0.5 * (os * cs - od * cd);
  }
}

// What a node adds to the sums of a step, each an (X, Y) pair: v[0] = m, the coefficient without w (c = m w);
// v[1..3] = dc / dp0, p1, p2;  v[4] = c + t dc/dt
template <int ENV, int MODE>
__host__ __device__ __forceinline__ void pulse_node_jac(const PulseLaunch &L, double p0, double p1, double p2, double w,
                                               bool axis_y, double t, double (&v)[5][2]) {
#pragma clang fp contract(off)
  double e[5], k[2], kt[2];
  pulse_envelope_jac<ENV>(p0, p1, p2, t, e);
  pulse_carrier_jac<MODE>(L, axis_y, t, k, kt);
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    v[0][a] = e[0] * k[a];
    v[1][a] = e[1] * k[a] * w;
    v[2][a] = e[2] * k[a] * w;
    v[3][a] = e[3] * k[a] * w;
    v[4][a] = (v[0][a] + t * (e[4] * k[a] + e[0] * kt[a])) * w;
  }
}

// R += A B
__host__ __device__ __forceinline__ void multiply_add(const CMat<2> &A, const CMat<2> &B, CMat<2> &R) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      double xr = R.re[2 * i + j], xi = R.im[2 * i + j];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        xr = fma(A.re[2 * i + k], B.re[2 * k + j], xr);
        xr = fma(-A.im[2 * i + k], B.im[2 * k + j], xr);
        xi = fma(A.re[2 * i + k], B.im[2 * k + j], xi);
        xi = fma(A.im[2 * i + k], B.re[2 * k + j], xi);
      }
      R.re[2 * i + j] = xr;
      R.im[2 * i + j] = xi;
    }
}
__host__ __device__ __forceinline__ void set_zero(CMat<2> &R) {
#pragma unroll
  for (int k = 0; k < 4; ++k) R.re[k] = R.im[k] = 0.0;
}

struct PulseJac {
  CMat<2> U, d[5];
};

// c = cos r, sinc = sin r / r and kappa = (cos r - sinc) / r^2 for r = sqrt(r2), the last two from their series where
// the quotient would cancel: what the derivative of exp(-i a . sigma) is made of (pulse_step_jac, exp_su2_jac)
__host__ __device__ __forceinline__ void sinc_kappa(double r2, double &c, double &sinc, double &kappa) {
  const double r = sqrt(r2);
  double s;
  sincos(r, &s, &c);
  const bool small = r < 0.05;
  sinc = small ? 1.0 - r2 * (1.0 / 6.0) * (1.0 - r2 * 0.05 * (1.0 - r2 * (1.0 / 42.0))) : s / r;
  kappa = small ? -1.0 / 3.0 + r2 * (1.0 / 30.0 - r2 * (1.0 / 840.0 - r2 * (1.0 / 45360.0 - r2 * (1.0 / 3991680.0))))
                : (c - sinc) / r2;
}

// U <- E U and d_k <- dE_k U + E d_k for E = exp(-i (gx X + gy Y)) and the directions (dgx[k], dgy[k]):
//   E = cos r I - i sinc (gx X + gy Y),  dE = -sinc rho I - i ((kappa rho gx + sinc dgx) X + (kappa rho gy + sinc dgy) Y)
// with rho = gx dgx + gy dgy and kappa = (cos r - sinc) / r^2, from its series where the difference would cancel.
// TANGENTS: bit k set = direction k is carried (the others stay zero).  false as pulse_step.
template <unsigned TANGENTS>
__host__ __device__ __forceinline__ bool pulse_step_jac(double gx, double gy, const double (&dgx)[5],
                                               const double (&dgy)[5], PulseJac &J) {
  const double r2 = gx * gx + gy * gy;
  double c, sinc, kappa;
  sinc_kappa(r2, c, sinc, kappa);
  CMat<2> E;
  E.re[0] = E.re[3] = c;
  E.re[1] = -sinc * gy;
  E.re[2] = sinc * gy;
  E.im[0] = E.im[3] = 0.0;
  E.im[1] = E.im[2] = -sinc * gx;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    if (!(TANGENTS >> k & 1u)) continue;
    const double rho = gx * dgx[k] + gy * dgy[k];
    const double vx = fma(kappa * rho, gx, sinc * dgx[k]), vy = fma(kappa * rho, gy, sinc * dgy[k]);
    CMat<2> dE, R;
    dE.re[0] = dE.re[3] = -sinc * rho;
    dE.re[1] = -vy;
    dE.re[2] = vy;
    dE.im[0] = dE.im[3] = 0.0;
    dE.im[1] = dE.im[2] = -vx;
    set_zero(R);
    multiply_add(dE, J.U, R);
    multiply_add(E, J.d[k], R);
    J.d[k] = R;
  }
  multiply_left(E, J.U);
  return fabs(gx) + fabs(gy) <= kEvolveMaxNorm;
}

// (P, dP_k) <- (L P, dL_k P + L dP_k) for the later partial product held `delta` lanes up: one tangent is fetched
// and folded at a time, so that beside the lane's own 48 doubles only L and one dL are alive
template <unsigned TANGENTS> __device__ __forceinline__ void combine_with_later_jac(PulseJac &J, int delta, int lanes) {
  CMat<2> Lm;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    Lm.re[k] = __shfl_down(J.U.re[k], delta, lanes);
    Lm.im[k] = __shfl_down(J.U.im[k], delta, lanes);
  }
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    if (!(TANGENTS >> t & 1u)) continue;
    CMat<2> dL, R;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dL.re[k] = __shfl_down(J.d[t].re[k], delta, lanes);
      dL.im[k] = __shfl_down(J.d[t].im[k], delta, lanes);
    }
    set_zero(R);
    multiply_add(dL, J.U, R);
    multiply_add(Lm, J.d[t], R);
    J.d[t] = R;
  }
  multiply_left(Lm, J.U);
}

// One work item per (solve, lane of the solve), as k_pulse_unitaries.
template <int ORDER, int ENV, int MODE>
__global__ __launch_bounds__(kEvolveThreads) void k_pulse_jac(const double *__restrict__ solves,
                                                                        const PulseLaunch L,
                                                                        double2 *__restrict__ out) {
  constexpr unsigned TANGENTS = ENV == kEnvDrag ? 0x1fu : 0x1bu;  // (no p2 without a third envelope parameter)
  constexpr bool kSupport = ENV == kEnvSquare || ENV == kEnvCosine;
  const int lanes = L.lanes, n_steps = L.n_steps;
  const auto [p0, p1, p2, w, T, axis_y, live, solve, lane, s_begin, s_end] = pulse_item(solves, L);
  const bool width_ends = kSupport && p1 < T;  // the grid ends at the width; a tie counts as T
  const double span = kSupport ? fmin(T, p1) : T;
  const double h = span / (double)n_steps, dh = 1.0 / (double)n_steps;
  const double dh_p1 = width_ends ? dh : 0.0, dh_T = width_ends ? 0.0 : dh;
  PulseJac J;
  set_identity(J.U);
#pragma unroll
  for (int k = 0; k < 5; ++k) set_zero(J.d[k]);
  bool ok = true;
  for (int s = s_begin; s < s_end; ++s) {
    double sa[5][2], sb[5][2];  // the weighted node sums of Omega_a and Omega_b (order 2: sa alone)
    if constexpr (ORDER == 2) {
      pulse_node_jac<ENV, MODE>(L, p0, p1, p2, w, axis_y, ((double)s + 0.5) * h, sa);
    } else {
#pragma unroll
      for (int k = 0; k < 5; ++k) sa[k][0] = sa[k][1] = sb[k][0] = sb[k][1] = 0.0;
#pragma nounroll  // (one copy of the transcendental code serves both nodes)
      for (int node = 0; node < 2; ++node) {
        double v[5][2];
        pulse_node_jac<ENV, MODE>(L, p0, p1, p2, w, axis_y, ((double)s + (node ? kC2 : kC1)) * h, v);
        const double wa = node ? kA2 : kA1, wb = node ? kA1 : kA2;
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            sa[k][a] = fma(wa, v[k][a], sa[k][a]);
            sb[k][a] = fma(wb, v[k][a], sb[k][a]);
          }
      }
    }
#pragma nounroll
    for (int half = 0; half < (ORDER == 4 ? 2 : 1); ++half) {  // Omega_a first, then Omega_b
      double g[2], dg[2][5];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        double m, d0, d1, d2, mv;
        if (ORDER == 4 && half) m = sb[0][a], d0 = sb[1][a], d1 = sb[2][a], d2 = sb[3][a], mv = sb[4][a];
        else m = sa[0][a], d0 = sa[1][a], d1 = sa[2][a], d2 = sa[3][a], mv = sa[4][a];
        g[a] = h * m * w;
        dg[a][0] = h * d0;
        dg[a][1] = fma(dh_p1, mv, h * d1);
        dg[a][2] = h * d2;
        dg[a][3] = h * m;
        dg[a][4] = dh_T * mv;
      }
      ok &= pulse_step_jac<TANGENTS>(g[0], g[1], dg[0], dg[1], J);
    }
  }
  int bad_run = ok ? 0 : 1;  // (folded beside the products: the p2 slot of a two-parameter envelope is not carried)
  for (int delta = 1; delta < lanes; delta <<= 1) {
    combine_with_later_jac<TANGENTS>(J, delta, lanes);
    bad_run |= __shfl_down(bad_run, delta, lanes);
  }
  if (!live || lane != 0) return;
  if (bad_run) {
    const double bad = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      J.U.re[k] = J.U.im[k] = bad;
#pragma unroll
      for (int t = 0; t < 5; ++t) J.d[t].re[k] = J.d[t].im[k] = bad;
    }
  }
  double2 *o = out + (size_t)solve * (kJacSlots * 4);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o[k] = make_double2(J.U.re[k], J.U.im[k]);
#pragma unroll
    for (int t = 0; t < 5; ++t) o[4 * (t + 1) + k] = make_double2(J.d[t].re[k], J.d[t].im[k]);
  }
}

// ---- the table-driven solve with directional derivatives ---------------------------------------------------------------
// k_evolve_magnus with the EXACT derivative of the grid's result in n_dirs directions (discretise, then differentiate,
// as k_pulse_jac).  A direction is a derivative of the coefficient table, dcoef[row][dir][node][term], and of the
// step, dh[row][dir]; per exponential factor Omega = h sum_j a_j A(t_j) it gives
//   dOmega = dh sum_j a_j A(t_j) + h sum_j a_j dA(t_j)
// (a moving node's f'(t_j) dt_j arrives inside dcoef: the kernel evaluates no function), and U <- E U,
// dU <- dE U + E dU.  One (row, direction) is one unit of work that recomputes U, so a direction's result does not
// depend on which others share the call; direction 0's unit stores U.
//
// DIM = 2: a lane holds U and dU (16 doubles); E = exp(-i (g0 I + a . sigma)) and dE in closed form (exp_su2_jac).
// DIM = 4: ONE COLUMN of U and dU per lane -- exp(Omega) U acts on columns independently, so the 4 neighbouring lanes
// of a unit's run share the exponent and never talk until the combine.  A lane that held the whole of U and dU beside
// both packed exponents and a column's series with its derivative would need near 280 live registers: one wave per SIMD.
// A column per lane needs 32 + 32 for the exponents and 48 for the series, stays under 256 VGPRs at two waves per SIMD
// and runs four times as many lanes; the price is that a unit's runs times 4 must fit a wave: lanes in {1, 4, 16}.
// The column's series carries its derivative term by term, v_{k+1} = Omega v_k / (k + 1), dv_{k+1} = (dOmega v_k +
// Omega dv_k) / (k + 1), with the cut and the term count of apply_exp (from nu of Omega alone); the parts of a cut
// exponent chain through (v, dv), which is the product rule across them.
// NC columns per lane, CL = DIM / NC lanes per run; u / d: column c of U / dU, entry i
template <int DIM, int NC> struct JacCols {
  double ur[NC][DIM], ui[NC][DIM], dr[NC][DIM], di[NC][DIM];
};

// E = exp(-i G) and its derivative in the direction dG, G = g0 I + a . sigma:  E = e^{-i g0} M,
//   M = cos r I - i sinc (a . sigma),  dM = -sinc rho I - i ((kappa rho a + sinc da) . sigma),  rho = a . da,
//   dE = e^{-i g0} (dM - i dg0 M)
__host__ __device__ __forceinline__ void exp_su2_jac(const Herm<2> &G, const Herm<2> &dG, CMat<2> &E, CMat<2> &dE) {
  const double g0 = 0.5 * (G.d[0] + G.d[1]), az = 0.5 * (G.d[0] - G.d[1]), ax = G.re[0], ay = -G.im[0];
  const double dg0 = 0.5 * (dG.d[0] + dG.d[1]), daz = 0.5 * (dG.d[0] - dG.d[1]), dax = dG.re[0], day = -dG.im[0];
  double c, sinc, kappa, ps, pc;
  sinc_kappa(ax * ax + ay * ay + az * az, c, sinc, kappa);
  sincos(g0, &ps, &pc);
  const double rho = ax * dax + ay * day + az * daz, kr = kappa * rho;
  const double vx = fma(kr, ax, sinc * dax), vy = fma(kr, ay, sinc * day), vz = fma(kr, az, sinc * daz);
  const double m_re[4] = {c, -sinc * ay, sinc * ay, c}, m_im[4] = {-sinc * az, -sinc * ax, -sinc * ax, sinc * az};
  const double n_re[4] = {-sinc * rho, -vy, vy, -sinc * rho}, n_im[4] = {-vz, -vx, -vx, vz};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double dr = fma(dg0, m_im[k], n_re[k]), di = fma(-dg0, m_re[k], n_im[k]);
    E.re[k] = pc * m_re[k] + ps * m_im[k];
    E.im[k] = pc * m_im[k] - ps * m_re[k];
    dE.re[k] = pc * dr + ps * di;
    dE.im[k] = pc * di - ps * dr;
  }
}

// (U, dU) <- (E U, dE U + E dU), E = exp(-i G) -> bit 0: G is not finite, bit 1: dG is not
__host__ __device__ __forceinline__ int step_jac(const Herm<2> &G, const Herm<2> &dG, JacCols<2, 2> &S) {
  CMat<2> E, dE;
  exp_su2_jac(G, dG, E, dE);
#pragma unroll
  for (int col = 0; col < 2; ++col) {
    double nur[2], nui[2], ndr[2], ndi[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      double xr = 0.0, xi = 0.0, yr = 0.0, yi = 0.0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double er = E.re[2 * i + k], ei = E.im[2 * i + k], fr = dE.re[2 * i + k], fi = dE.im[2 * i + k];
        xr = fma(er, S.ur[col][k], xr), xr = fma(-ei, S.ui[col][k], xr);
        xi = fma(er, S.ui[col][k], xi), xi = fma(ei, S.ur[col][k], xi);
        yr = fma(fr, S.ur[col][k], yr), yr = fma(-fi, S.ui[col][k], yr);
        yi = fma(fr, S.ui[col][k], yi), yi = fma(fi, S.ur[col][k], yi);
        yr = fma(er, S.dr[col][k], yr), yr = fma(-ei, S.di[col][k], yr);
        yi = fma(er, S.di[col][k], yi), yi = fma(ei, S.dr[col][k], yi);
      }
      nur[i] = xr, nui[i] = xi, ndr[i] = yr, ndi[i] = yi;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) S.ur[col][i] = nur[i], S.ui[col][i] = nui[i], S.dr[col][i] = ndr[i], S.di[col][i] = ndi[i];
  }
  const double ng = fabs(G.d[0]) + fabs(G.d[1]) + fabs(G.re[0]) + fabs(G.im[0]);
  const double nd = fabs(dG.d[0]) + fabs(dG.d[1]) + fabs(dG.re[0]) + fabs(dG.im[0]);
  return (ng <= 1.7e308 ? 0 : 1) | (nd <= 1.7e308 ? 0 : 2);
}

// the lane's column: (v, dv) <- (exp(-i G) v, d exp(-i G) v + exp(-i G) dv) by the series of apply_exp with its
// derivative -> bit 0: the norm of G is not finite or beyond kEvolveMaxNorm (nothing is changed), bit 1: dG is not finite
__host__ __device__ __forceinline__ int step_jac(const Herm<4> &G, const Herm<4> &dG, JacCols<4, 1> &S) {
  const SeriesCut cut = series_cut(G);
  const int bad_d = herm_row_norm(dG) <= 1.7e308 ? 0 : 2;
  if (!cut.ok) return 1 | bad_d;
  const int parts = cut.parts, n_series = cut.n_series;
  const double inv_parts = cut.inv_parts;
  for (int p = 0; p < parts; ++p) {
    double tr[4], ti[4], er[4], ei[4];  // the running term and its derivative
#pragma unroll
    for (int i = 0; i < 4; ++i) tr[i] = S.ur[0][i], ti[i] = S.ui[0][i], er[i] = S.dr[0][i], ei[i] = S.di[0][i];
    for (int k = 1; k <= n_series; ++k) {
      double yr[4], yi[4], zr[4], zi[4];
      herm_matvec(dG, tr, ti, zr, zi);
      herm_matvec<true>(G, er, ei, zr, zi);
      herm_matvec(G, tr, ti, yr, yi);
      const double f = inv_parts / (double)k;  // term <- (-i G / parts) term / k
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        tr[i] = f * yi[i], ti[i] = -f * yr[i];
        er[i] = f * zi[i], ei[i] = -f * zr[i];
        S.ur[0][i] += tr[i], S.ui[0][i] += ti[i];
        S.dr[0][i] += er[i], S.di[0][i] += ei[i];
      }
    }
  }
  return bad_d;
}

// (P, dP) <- (L P, dL P + L dP) for the later partial product (L, dL), held by the CL lanes that start delta * CL
// lanes up.  Entry (i, k) of L sits in lane k / NC of them, column k % NC: every lane reads the 4 * DIM * DIM doubles
// it needs, then overwrites its own.  A lane whose later run lies outside its unit reads another unit's and ends with
// a product nobody uses (as combine_with_later: lanes is a power of two and run 0 only ever reads runs that are whole).
template <int DIM, int NC> __device__ __forceinline__ void combine_with_later_jac(JacCols<DIM, NC> &S, int delta) {
  constexpr int CL = DIM / NC;
  const int wave_lane = (int)(threadIdx.x & (kWave - 1)), first = wave_lane - (wave_lane & (CL - 1)) + delta * CL;
  JacCols<DIM, NC> R;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < DIM; ++i) R.ur[c][i] = R.ui[c][i] = R.dr[c][i] = R.di[c][i] = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const int src = (first + k / NC) & (kWave - 1);
      const double lr = __shfl(S.ur[k % NC][i], src), li = __shfl(S.ui[k % NC][i], src);
      const double mr = __shfl(S.dr[k % NC][i], src), mi = __shfl(S.di[k % NC][i], src);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        R.ur[c][i] = fma(lr, S.ur[c][k], R.ur[c][i]), R.ur[c][i] = fma(-li, S.ui[c][k], R.ur[c][i]);
        R.ui[c][i] = fma(lr, S.ui[c][k], R.ui[c][i]), R.ui[c][i] = fma(li, S.ur[c][k], R.ui[c][i]);
        R.dr[c][i] = fma(mr, S.ur[c][k], R.dr[c][i]), R.dr[c][i] = fma(-mi, S.ui[c][k], R.dr[c][i]);
        R.di[c][i] = fma(mr, S.ui[c][k], R.di[c][i]), R.di[c][i] = fma(mi, S.ur[c][k], R.di[c][i]);
        R.dr[c][i] = fma(lr, S.dr[c][k], R.dr[c][i]), R.dr[c][i] = fma(-li, S.di[c][k], R.dr[c][i]);
        R.di[c][i] = fma(lr, S.di[c][k], R.di[c][i]), R.di[c][i] = fma(li, S.dr[c][k], R.di[c][i]);
      }
    }
  S = R;
}

// One work item per (row, direction, run of the steps, column lane); a block holds kEvolveThreads / (lanes * CL) units.
template <int DIM, int ORDER>
__global__ __launch_bounds__(kEvolveThreads) void k_evolve_magnus_jac(const EvolveTerms terms, int n_terms,
                                                                      const double *__restrict__ coef,
                                                                      const double *__restrict__ h_rows,
                                                                      const double *__restrict__ dcoef,
                                                                      const double *__restrict__ dh_rows, int rows,
                                                                      int n_dirs, int n_steps, int lanes,
                                                                      double2 *__restrict__ out) {
  constexpr int NC = DIM == 2 ? 2 : 1, CL = DIM / NC, NODES = ORDER == 4 ? 2 : 1;
  const long long gid = (long long)blockIdx.x * kEvolveThreads + threadIdx.x;
  const int col_lane = (int)(gid & (CL - 1));
  const long long item = gid / CL, unit_ll = item / lanes, n_units = (long long)rows * n_dirs;
  const int run = (int)(item - unit_ll * lanes);
  const bool live = unit_ll < n_units;  // (a unit's lanes are live or idle together: lanes * CL divides the block)
  const int unit = (int)(live ? unit_ll : n_units - 1), row = unit / n_dirs, dir = unit - row * n_dirs;
  const int s_begin = (int)((long long)run * n_steps / lanes), s_end = (int)((long long)(run + 1) * n_steps / lanes);
  const double h = h_rows[row], dh = dh_rows[unit];
  const size_t node_stride = (size_t)NODES * n_terms;
  const double *__restrict__ c = coef + ((size_t)row * n_steps + s_begin) * node_stride;
  const double *__restrict__ dc = dcoef + ((size_t)unit * n_steps + s_begin) * node_stride;
  JacCols<DIM, NC> S;
#pragma unroll
  for (int k = 0; k < NC; ++k)
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      S.ur[k][i] = (i == col_lane * NC + k) ? 1.0 : 0.0;
      S.ui[k][i] = S.dr[k][i] = S.di[k][i] = 0.0;
    }
  Herm<DIM> G, dG;
  int bad = 0;
  for (int s = s_begin; s < s_end; ++s, c += node_stride, dc += node_stride) {
    if constexpr (ORDER == 2) {
      weighted_sum<DIM>(terms, n_terms, c, nullptr, h, 0.0, G);
      weighted_sum<DIM>(terms, n_terms, c, nullptr, dh, 0.0, dG);
      weighted_add<DIM>(terms, n_terms, dc, nullptr, h, 0.0, dG);
      bad |= step_jac(G, dG, S);
    } else {
#pragma nounroll
      for (int half = 0; half < 2; ++half) {  // Omega_a first, then Omega_b: the weights exchanged
        const double w1 = half ? kA2 : kA1, w2 = half ? kA1 : kA2;
        weighted_sum<DIM>(terms, n_terms, c, c + n_terms, h * w1, h * w2, G);
        weighted_sum<DIM>(terms, n_terms, c, c + n_terms, dh * w1, dh * w2, dG);
        weighted_add<DIM>(terms, n_terms, dc, dc + n_terms, h * w1, h * w2, dG);
        bad |= step_jac(G, dG, S);
      }
    }
  }
  for (int delta = 1; delta < lanes; delta <<= 1) {  // run 0 ends with the unit
    combine_with_later_jac(S, delta);
    bad |= __shfl(bad, (int)((threadIdx.x + delta * CL) & (kWave - 1)));
  }
  if (!live || run != 0) return;
  const double nan = __builtin_nan("");
  double2 *__restrict__ o = out + (size_t)row * (1 + n_dirs) * (DIM * DIM);
  double2 *__restrict__ od = o + (size_t)(1 + dir) * (DIM * DIM);
#pragma unroll
  for (int k = 0; k < NC; ++k)
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const int e = i * DIM + col_lane * NC + k;
      if (dir == 0) o[e] = (bad & 1) ? make_double2(nan, nan) : make_double2(S.ur[k][i], S.ui[k][i]);
      od[e] = bad ? make_double2(nan, nan) : make_double2(S.dr[k][i], S.di[k][i]);
    }
}

// ---- 8x8 and 16x16: the table-driven solve on three and four wires -----------------------------------------------------
// k_evolve_magnus's scheme, node order, norm rule and series cut (series_cut_norm) at DIM = 8 and 16, where neither U
// nor the exponent fits a lane's registers.  ONE COLUMN of U per lane, as k_evolve_magnus_jac at DIM = 4: exp(Omega) U
// acts on columns independently, so the DIM neighbouring lanes of a run of steps share the exponent and differ in
// their column.  The exponent G = h sum_j a_j sum_i c_i(t_j) H_i of the current factor lives in LDS, one region per
// run: lane c of the run forms row c -- from the real diagonal and the entries above it, the rest by conjugation, so G
// is Hermitian to the bit --, stores the part on and above the diagonal (packed, DIM (DIM + 1) / 2 complex128) and
// reports its absolute row sum; the largest of the run is the norm.  The terms come from device memory,
// [n_terms][DIM][DIM] complex128: 16 of them are 64 KiB at DIM = 16.
// Registers.  A lane keeps its column v and the running Taylor term t (2 DIM doubles each) and forms the next term row
// by row, reading G at addresses its run shares.  At DIM = 16 three such vectors, the reads in flight and the
// addresses do not fit the 256 registers of two waves per SIMD, so the upper half of the next term is parked in the
// run's region behind G (one 16-byte slot per lane and row, lanes adjacent) until the product is complete: v, t and
// half a term stay in registers.  The packed G is what makes room for that: 8 runs x (136 + 128 + 1) x 16 bytes are
// 33 KiB per workgroup of 128 threads, four workgroups per CU.  The regions are one element apart from a multiple of
// the bank cycle, so the runs of a wave read different banks.
// Combine: a run writes its partial product into its region, column by column, as a plain DIM x DIM matrix (the
// region holds one); run r then multiplies the matrix of run r + delta of its own row onto its column -- log2(lanes)
// rounds, later run on the left; a run without such a partner in a round sits the multiplication out.
// A run's lanes and the runs of a row share a wave (lanes * DIM <= 64), the lanes of a run take the same branches
// (the cut follows from the shared norm), and nothing in LDS is shared between waves: the build, the series and the
// combine are ordered by wave-level fences, never by a workgroup barrier -- runs of unequal length and rows of unequal
// norm sit in one workgroup.
constexpr int kWideThreads = 128;

template <int DIM> struct WideLds {
  static constexpr int KEEP = DIM > 8 ? DIM / 2 : DIM;     // rows of the next term that stay in registers
  static constexpr int PACKED = DIM * (DIM + 1) / 2;       // G on and above the diagonal
  static constexpr int STAGE = PACKED;                     // the parked rows start here: [(i - KEEP) * DIM + column]
  static constexpr int USED = PACKED + (DIM - KEEP) * DIM;
  static constexpr int REGION = (USED > DIM * DIM ? USED : DIM * DIM) + 1;
  static constexpr int RUNS = kWideThreads / DIM;
  // entry (i, j), i <= j, of the packed G
  static constexpr int at(int i, int j) { return i * DIM - i * (i - 1) / 2 + (j - i); }
};

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Row `c` of G = sum_i w_i H_i: its entries from the diagonal on into the run's region -> its absolute row sum (the
// norm rule of herm_row_norm)
template <int DIM>
__device__ __forceinline__ double wide_build_row(const double2 *__restrict__ terms, int n_terms, const double *__restrict__ c0,
                                                 const double *__restrict__ c1, double w0, double w1, int c, double2 *G) {
  double gr[DIM], gi[DIM];
#pragma unroll
  for (int j = 0; j < DIM; ++j) gr[j] = gi[j] = 0.0;
  for (int t = 0; t < n_terms; ++t) {
    double w = w0 * c0[t];
    if (c1) w = fma(w1, c1[t], w);
    const double2 *__restrict__ H = terms + (size_t)t * (DIM * DIM);
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      const int at = j >= c ? c * DIM + j : j * DIM + c;  // on and above the diagonal as stored, below: the conjugate
      const double2 e = H[at];
      gr[j] = fma(w, e.x, gr[j]);
      gi[j] = j == c ? 0.0 : fma(j > c ? w : -w, e.y, gi[j]);
    }
  }
  double row = 0.0;
  double2 *mine = G + (c * DIM - c * (c - 1) / 2 - c);  // entry (c, j) at mine[j]
#pragma unroll
  for (int j = 0; j < DIM; ++j) {
    row += fabs(gr[j]) + fabs(gi[j]);
    if (j >= c) mine[j] = make_double2(gr[j], gi[j]);
  }
  return row;
}

// the lane's column: v <- exp(-i G) v for the run's packed G, by the series of apply_exp -> false (nothing changed)
// when the norm is not finite or beyond kEvolveMaxNorm
template <int DIM>
__device__ __forceinline__ bool wide_step(double2 *G, int col, double row_sum, double (&vr)[DIM], double (&vi)[DIM]) {
  using W = WideLds<DIM>;
  double nu = row_sum;
#pragma unroll
  for (int m = 1; m < DIM; m <<= 1) {  // the largest of the run's DIM lanes (a NaN stays)
    const double o = __shfl_xor(nu, m, kWave);
    nu = (o > nu || o != o) ? o : nu;
  }
  const SeriesCut cut = series_cut_norm(nu);
  if (!cut.ok) return false;
  double2 *stage = G + W::STAGE + col;
  for (int p = 0; p < cut.parts; ++p) {
    // the running term: rows below KEEP in registers, the others in the lane's parked slots (every round reads
    // them from there, the first one included: one form of the loop, no pointer that is a register in one round
    // and LDS in the next)
    double tr[DIM], ti[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      if (i < W::KEEP) tr[i] = vr[i], ti[i] = vi[i];
      else stage[(i - W::KEEP) * DIM] = make_double2(vr[i], vi[i]);
    }
    for (int k = 1; k <= cut.n_series; ++k) {
      const double f = cut.inv_parts / (double)k;  // term <- (-i G / parts) term / k
#pragma unroll
      for (int i = W::KEEP; i < DIM; ++i) {
        const double2 a = stage[(i - W::KEEP) * DIM];
        tr[i] = a.x, ti[i] = a.y;
      }
      double nr[W::KEEP], ni[W::KEEP];
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        double xr = 0.0, xi = 0.0;
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
          const double2 g = G[i <= j ? W::at(i, j) : W::at(j, i)];
          const double gy = i <= j ? g.y : -g.y;
          xr = fma(g.x, tr[j], xr);
          xr = fma(-gy, ti[j], xr);
          xi = fma(g.x, ti[j], xi);
          xi = fma(gy, tr[j], xi);
        }
        const double ar = f * xi, ai = -f * xr;
        vr[i] += ar;
        vi[i] += ai;
        if (i < W::KEEP) nr[i < W::KEEP ? i : 0] = ar, ni[i < W::KEEP ? i : 0] = ai;  // (no index beyond the array, dead or not)
        else stage[(i - W::KEEP) * DIM] = make_double2(ar, ai);
        // (a row's reads stay with its row: hoisted, the DIM * DIM reads of a product spill)
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < W::KEEP; ++i) tr[i] = nr[i], ti[i] = ni[i];
    }
  }
  return true;
}

// One work item per (row, run of the steps, column lane); a block holds kWideThreads / (lanes * DIM) rows.
template <int DIM, int ORDER>
__global__ __launch_bounds__(kWideThreads, 2) void k_evolve_wide(const double2 *__restrict__ terms, int n_terms,
                                                                 const double *__restrict__ coef,
                                                                 const double *__restrict__ h_rows, int rows, int n_steps,
                                                                 int lanes, double2 *__restrict__ out) {
  using W = WideLds<DIM>;
  constexpr int NODES = ORDER == 4 ? 2 : 1;
  __shared__ double2 lds[W::RUNS * W::REGION];
  const long long gid = (long long)blockIdx.x * kWideThreads + threadIdx.x;
  const int col = (int)(gid & (DIM - 1));
  const long long item = gid / DIM, row_ll = item / lanes;
  const int run = (int)(item - row_ll * lanes), block_run = (int)(threadIdx.x / DIM);
  const bool live = row_ll < rows;  // (a row's lanes are live or idle together: lanes * DIM divides the block)
  const int row = live ? (int)row_ll : rows - 1;
  const int s_begin = (int)((long long)run * n_steps / lanes), s_end = (int)((long long)(run + 1) * n_steps / lanes);
  const double h = h_rows[row];
  const size_t node_stride = (size_t)NODES * n_terms;
  const double *__restrict__ c = coef + ((size_t)row * n_steps + s_begin) * node_stride;
  double2 *G = lds + block_run * W::REGION;
  double vr[DIM], vi[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) vr[i] = i == col ? 1.0 : 0.0, vi[i] = 0.0;
  int bad = 0;
  for (int s = s_begin; s < s_end; ++s, c += node_stride) {
#pragma nounroll
    for (int half = 0; half < NODES; ++half) {  // order 4: Omega_a first, then Omega_b -- the weights exchanged
      const double w1 = ORDER == 2 ? h : h * (half ? kA2 : kA1), w2 = h * (half ? kA1 : kA2);
      wave_lds_fence();  // (the run has finished reading the previous factor)
      const double row_sum = wide_build_row<DIM>(terms, n_terms, c, ORDER == 4 ? c + n_terms : nullptr, w1, w2, col, G);
      wave_lds_fence();
      bad |= wide_step<DIM>(G, col, row_sum, vr, vi) ? 0 : 1;
    }
  }
  for (int delta = 1; delta < lanes; delta <<= 1) {  // run 0 ends with the row
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < DIM; ++i) G[i * DIM + col] = make_double2(vr[i], vi[i]);
    wave_lds_fence();
    // only a run whose later run lies inside its row multiplies: that run shares its wave, so the fences above order
    // its columns before these reads; the others keep a product nobody uses (the predicate is uniform across a run)
    const bool in_row = run + delta < lanes;
    const int later_bad = __shfl(bad, (int)((threadIdx.x + delta * DIM) & (kWave - 1)));
    if (in_row) {
      const double2 *L = lds + (block_run + delta) * W::REGION;
      double yr[DIM], yi[DIM];
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        double xr = 0.0, xi = 0.0;
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
          const double2 g = L[i * DIM + j];
          xr = fma(g.x, vr[j], xr);
          xr = fma(-g.y, vi[j], xr);
          xi = fma(g.x, vi[j], xi);
          xi = fma(g.y, vr[j], xi);
        }
        yr[i] = xr;
        yi[i] = xi;
        __builtin_amdgcn_sched_barrier(0);  // (as in wide_step)
      }
#pragma unroll
      for (int i = 0; i < DIM; ++i) vr[i] = yr[i], vi[i] = yi[i];
      bad |= later_bad;
    }
  }
  if (!live || run != 0) return;
  const double nan = __builtin_nan("");
  double2 *__restrict__ o = out + (size_t)row * (DIM * DIM);
#pragma unroll
  for (int i = 0; i < DIM; ++i) o[i * DIM + col] = bad ? make_double2(nan, nan) : make_double2(vr[i], vi[i]);
}

// ---- composition of small circuits ------------------------------------------------------------------------------------
// The product rule of qoc.circuit_unitaries on the device: per circuit and candidate U = I, dU_p = 0 and per op
// dU_p <- M dU_p + dM_p U, U <- M U.  Left multiplication acts on every column on its own and dU_p needs only U and
// itself, so ONE lane carries column j of U and of ONE dU_p (or of none: the "U only" lane q = 0) -- 2 x DIM complex
// numbers -- and recomputes its U column beside the P other lanes that hold the same one.  The lanes of a circuit are
// ordered (candidate, q, column) with the column fastest and every circuit starts at a multiple of 4 lanes, so the DIM
// lanes of one (candidate, q) are neighbours inside a wave: the column sum of the overlap is DIM lane reads in a fixed
// order.  A lane's parameter selects its tangent terms by comparison and select (lanes of different p share a wave);
// what branches is the op's kind and placement, which every lane of a circuit shares.  DIM is a template parameter
// and every loop over matrix entries is unrolled: no private array is indexed at run time.
struct ComposeLaunch {
  const qmle_compose_circuit *circuits;
  const qmle_compose_op *ops;
  const qmle_compose_term *terms;
  const int32_t *rows;
  const long long *lane_begin;  // [n_circuits + 1], multiples of 4
  const double2 *mats;
  const double *coefs;
  const double2 *targets;
  const double2 *jac;
  double2 *ov, *full;
  int n_circuits, n_candidates;
  unsigned column_mask;
};

// acc += a b
__device__ __forceinline__ void cfma(const double2 a, const double2 b, double2 &acc) {
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(-a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(a.y, b.x, acc.y);
}
__device__ __forceinline__ double2 cselect(bool take, const double2 a, const double2 b) {
  return make_double2(take ? a.x : b.x, take ? a.y : b.y);
}

template <int DIM>
__device__ __forceinline__ void compose_lane(const ComposeLaunch &L, const qmle_compose_circuit K, int c, int q, int j,
                                             bool live) {
  const int p = q - 1, P = K.n_params;
  const double2 zero = make_double2(0.0, 0.0);
  double2 u[DIM], du[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    u[i] = make_double2(i == j ? 1.0 : 0.0, 0.0);
    du[i] = zero;
  }
  for (int oi = K.op_begin; oi < K.op_end; ++oi) {
    const qmle_compose_op o = L.ops[oi];
    const bool pulse = o.kind == QMLE_COMPOSE_PULSE;
    const double2 *__restrict__ mp =
        pulse ? L.jac + (size_t)L.rows[o.mat_off + c] * (kJacSlots * 4) : L.mats + (o.mat_off + (long long)c * o.mat_stride);
    const bool has_terms = o.term_end > o.term_begin;
    if (DIM == 4 && (o.placement == 1 || o.placement == 4)) {  // the other wire order: exchange |01> and |10>
      const double2 a = u[1 % DIM], b = du[1 % DIM];
      u[1 % DIM] = u[2 % DIM], u[2 % DIM] = a;
      du[1 % DIM] = du[2 % DIM], du[2 % DIM] = b;
    }
    if (DIM == 2 || o.placement <= 2) {  // a 2 x 2 matrix on one wire (of DIM = 4: on the pairs (0, 1) and (2, 3))
      double2 m[4], dm[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = mp[k], dm[k] = zero;
      if (has_terms) {
        if (pulse) {
          for (int t = o.term_begin; t < o.term_end; ++t) {
            const qmle_compose_term T = L.terms[t];
            const bool mine = T.param == p;
            const double w = L.coefs[T.coef_off + c];
            const double2 *__restrict__ g = mp + 4 * (1 + T.slot);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const double2 v = g[k];
              dm[k].x += mine ? w * v.x : 0.0;
              dm[k].y += mine ? w * v.y : 0.0;
            }
          }
        } else {  // (-i/2) sigma M, weighted by the sum of this lane's coefficients
          double w = 0.0;
          for (int t = o.term_begin; t < o.term_end; ++t) {
            const qmle_compose_term T = L.terms[t];
            w += T.param == p ? L.coefs[T.coef_off + c] : 0.0;
          }
          const double h = 0.5 * w;
          if (o.kind == QMLE_COMPOSE_ROT_X) {  // -i/2 (m1; m0)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              dm[k] = make_double2(h * m[2 + k].y, -h * m[2 + k].x);
              dm[2 + k] = make_double2(h * m[k].y, -h * m[k].x);
            }
          } else if (o.kind == QMLE_COMPOSE_ROT_Y) {  // 1/2 (-m1; m0)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              dm[k] = make_double2(-h * m[2 + k].x, -h * m[2 + k].y);
              dm[2 + k] = make_double2(h * m[k].x, h * m[k].y);
            }
          } else {  // i/2 (-m0; m1)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              dm[k] = make_double2(h * m[k].y, -h * m[k].x);
              dm[2 + k] = make_double2(-h * m[2 + k].y, h * m[2 + k].x);
            }
          }
        }
      }
#pragma unroll
      for (int b = 0; b < DIM; b += 2) {
        double2 n0 = zero, n1 = zero, d0 = zero, d1 = zero;
        cfma(m[0], du[b], d0), cfma(m[1], du[b + 1], d0);
        cfma(m[2], du[b], d1), cfma(m[3], du[b + 1], d1);
        if (has_terms) {
          cfma(dm[0], u[b], d0), cfma(dm[1], u[b + 1], d0);
          cfma(dm[2], u[b], d1), cfma(dm[3], u[b + 1], d1);
        }
        cfma(m[0], u[b], n0), cfma(m[1], u[b + 1], n0);
        cfma(m[2], u[b], n1), cfma(m[3], u[b + 1], n1);
        u[b] = n0, u[b + 1] = n1, du[b] = d0, du[b + 1] = d1;
      }
    } else if constexpr (DIM == 4) {  // a 4 x 4 matrix on both wires
      double2 m[16], nu[4], nd[4];
#pragma unroll
      for (int k = 0; k < 16; ++k) m[k] = mp[k];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        nu[a] = nd[a] = zero;
#pragma unroll
        for (int b = 0; b < 4; ++b) cfma(m[4 * a + b], u[b], nu[a]), cfma(m[4 * a + b], du[b], nd[a]);
      }
      if (has_terms) {  // CPHASE: i |11><11| M, weighted: row 3 alone
        double w = 0.0;
        for (int t = o.term_begin; t < o.term_end; ++t) {
          const qmle_compose_term T = L.terms[t];
          w += T.param == p ? L.coefs[T.coef_off + c] : 0.0;
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) cfma(make_double2(-w * m[12 + b].y, w * m[12 + b].x), u[b], nd[3]);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) u[a] = nu[a], du[a] = nd[a];
    }
    if (DIM == 4 && (o.placement == 1 || o.placement == 4)) {
      const double2 a = u[1 % DIM], b = du[1 % DIM];
      u[1 % DIM] = u[2 % DIM], u[2 % DIM] = a;
      du[1 % DIM] = du[2 % DIM], du[2 % DIM] = b;
    }
  }
  const bool u_lane = q == 0;
  // the overlap with the target: this lane's column, then the DIM columns in index order
  const bool with_target = K.target_off >= 0 && L.ov != nullptr;
  double2 part = zero;
  if (with_target) {
    const double2 *__restrict__ V = L.targets + K.target_off;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double2 v = V[i * DIM + j];
      cfma(make_double2(v.x, -v.y), cselect(u_lane, u[i], du[i]), part);
    }
  }
  part = cselect((L.column_mask >> j & 1u) != 0, part, zero);
  const int first = (int)(threadIdx.x & (kWave - 1)) - j;
  double2 sum = zero;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    sum.x += __shfl(part.x, first + k);
    sum.y += __shfl(part.y, first + k);
  }
  if (!live) return;
  if (with_target && j == 0) {
    if (u_lane) L.ov[K.ov_off + c] = sum;
    else L.ov[K.dov_off + (long long)c * P + p] = sum;
  }
  if (L.full != nullptr) {
    double2 *__restrict__ out =
        L.full + (u_lane ? K.u_off + (long long)c * (DIM * DIM) : K.du_off + ((long long)c * P + p) * (DIM * DIM));
#pragma unroll
    for (int i = 0; i < DIM; ++i) out[i * DIM + j] = cselect(u_lane, u[i], du[i]);
  }
}

__global__ __launch_bounds__(kEvolveThreads) void k_compose_circuits(const ComposeLaunch L) {
  const long long gid = (long long)blockIdx.x * kEvolveThreads + threadIdx.x;
  int lo = 0, hi = L.n_circuits;  // the circuit k with lane_begin[k] <= gid < lane_begin[k + 1] (the last one past the end)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (L.lane_begin[mid] <= gid) lo = mid;
    else hi = mid;
  }
  const qmle_compose_circuit K = L.circuits[lo];
  const int dim = 1 << K.n_wires;
  const long long local = gid - L.lane_begin[lo];
  const int j = (int)(local & (dim - 1));
  const long long item = local / dim;
  const int q = (int)(item % (K.n_params + 1));
  const long long c_ll = item / (K.n_params + 1);
  const bool live = c_ll < L.n_candidates;  // (padding lanes redo the last candidate and store nothing)
  const int c = live ? (int)c_ll : L.n_candidates - 1;
  if (dim == 2) compose_lane<2>(L, K, c, q, j, live);
  else compose_lane<4>(L, K, c, q, j, live);
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

// the allowed lanes_per_row of the wide solve: a row's runs times DIM column lanes share a wave
bool wide_lanes_allowed(int dim, int lanes) { return lanes == 1 || lanes == 4 || (lanes == 8 && dim == 8); }
// lanes_per_row = 0, as evolve_auto_lanes: the widest allowed split that stays within the card's lanes and leaves
// every run a step
int evolve_wide_auto_lanes(int rows, int n_steps, int dim) {
  const long long fill = 256ll * 4 * 2 * kWave;
  int lanes = 1;
  for (int cand : {4, 8})
    if (wide_lanes_allowed(dim, cand) && (long long)rows * cand * dim <= fill && cand <= n_steps) lanes = cand;
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

// the lanes of a row (lanes_per_row, 0 = evolve_auto_lanes) and the grid of one work item per (row, lane); false for
// another lane count or more blocks than grid.x holds.  rows and n_steps are >= 1.
bool evolve_launch_shape(int rows, int n_steps, int lanes_per_row, int &lanes, dim3 &grid) {
  if (lanes_per_row != 0 && lanes_per_row != 1 && lanes_per_row != 4 && lanes_per_row != 16 && lanes_per_row != 64)
    return false;
  lanes = lanes_per_row ? lanes_per_row : evolve_auto_lanes(rows, n_steps);
  const long long items = (long long)rows * lanes;
  grid = dim3(grid_for((uint64_t)items, kEvolveThreads));
  return items <= (1ll << 31) - kEvolveThreads;
}

// what both pulse entry points refuse (QMLE_OK or the error code), then L.lanes and the grid
int pulse_launch(const double *d_solves, const void *d_out, int order, int lanes_per_solve, PulseLaunch &L, dim3 &grid) {
  if (order != 2 && order != 4) return QMLE_ERR_UNSUPPORTED;
  if (L.envelope < 0 || L.envelope >= kEnvCount || L.mode < 0 || L.mode >= kModeCount) return QMLE_ERR_UNSUPPORTED;
  if (!d_solves || !d_out || L.n_solves < 1 || L.n_steps < 1 || !(fabs(L.omega_c) <= 1e300) || !(fabs(L.omega_q) <= 1e300))
    return QMLE_ERR_INVALID_ARG;
  return evolve_launch_shape(L.n_solves, L.n_steps, lanes_per_solve, L.lanes, grid) ? QMLE_OK : QMLE_ERR_INVALID_ARG;
}

// f(order, envelope, mode) with the three run-time values as std::integral_constant, for the kernels' template arguments
template <int V> using Int = std::integral_constant<int, V>;
template <class F> void dispatch_pulse(int order, int envelope, int mode, F f) {
  auto by_mode = [&](auto o, auto e) {
    if (mode == kModeRwa) f(o, e, Int<kModeRwa>{});
    else if (mode == kModeLab) f(o, e, Int<kModeLab>{});
    else f(o, e, Int<kModeDrive>{});
  };
  auto by_envelope = [&](auto o) {
    switch (envelope) {
      case kEnvGaussian: by_mode(o, Int<kEnvGaussian>{}); break;
      case kEnvSquare: by_mode(o, Int<kEnvSquare>{}); break;
      case kEnvCosine: by_mode(o, Int<kEnvCosine>{}); break;
      case kEnvDrag: by_mode(o, Int<kEnvDrag>{}); break;
      default: by_mode(o, Int<kEnvSech>{}); break;
    }
  };
  if (order == 2) by_envelope(Int<2>{});
  else by_envelope(Int<4>{});
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
  if ((long long)n_steps * (order == 4 ? 2 : 1) * n_terms > (1ll << 31) - 1) return QMLE_ERR_INVALID_ARG;
  int lanes;
  dim3 grid;
  if (!evolve_launch_shape(rows, n_steps, lanes_per_row, lanes, grid)) return QMLE_ERR_INVALID_ARG;
  EvolveTerms T;
  if (dim == 2) pack_terms<2>(h_terms, n_terms, T);
  else pack_terms<4>(h_terms, n_terms, T);
  for (int t = n_terms; t < kEvolveMaxTerms; ++t)
    for (int k = 0; k < 16; ++k) T.h[t][k] = 0.0;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 block(kEvolveThreads);
#define QMLE_EVOLVE_LAUNCH(D, O)                                                                                \
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

int qmle_evolve_wide_lanes(int rows, int n_steps, int dim) {
  if (dim != 8 && dim != 16) return QMLE_ERR_UNSUPPORTED;
  if (rows < 1 || n_steps < 1) return QMLE_ERR_INVALID_ARG;
  return evolve_wide_auto_lanes(rows, n_steps, dim);
}

int qmle_evolve_magnus_wide(const void *d_terms, int n_terms, int dim, const double *d_coef, const double *d_h, int rows,
                            int order, int n_steps, int lanes_per_row, void *d_out, qmle_stream stream_) {
  if (dim != 8 && dim != 16) return QMLE_ERR_UNSUPPORTED;
  if (order != 2 && order != 4) return QMLE_ERR_UNSUPPORTED;
  if (!d_terms || !d_coef || !d_h || !d_out || n_terms < 1 || n_terms > kEvolveMaxTerms || rows < 1 || n_steps < 1)
    return QMLE_ERR_INVALID_ARG;
  if ((long long)n_steps * (order == 4 ? 2 : 1) * n_terms > (1ll << 31) - 1) return QMLE_ERR_INVALID_ARG;
  if (lanes_per_row != 0 && !wide_lanes_allowed(dim, lanes_per_row)) return QMLE_ERR_INVALID_ARG;
  const int lanes = lanes_per_row ? lanes_per_row : evolve_wide_auto_lanes(rows, n_steps, dim);
  const long long items = (long long)rows * lanes * dim;
  if (items > (1ll << 31) - kWideThreads) return QMLE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(grid_for((uint64_t)items, kWideThreads)), block(kWideThreads);
#define QMLE_EVOLVE_LAUNCH(D, O)                                                                                   \
  hipLaunchKernelGGL((k_evolve_wide<D, O>), grid, block, 0, stream, (const double2 *)d_terms, n_terms, d_coef, d_h, \
                     rows, n_steps, lanes, (double2 *)d_out)
  if (dim == 8 && order == 2) QMLE_EVOLVE_LAUNCH(8, 2);
  else if (dim == 8) QMLE_EVOLVE_LAUNCH(8, 4);
  else if (order == 2) QMLE_EVOLVE_LAUNCH(16, 2);
  else QMLE_EVOLVE_LAUNCH(16, 4);
#undef QMLE_EVOLVE_LAUNCH
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_evolve_magnus_jac(const double *h_terms, int n_terms, int dim, const double *d_coef, const double *d_h,
                           const double *d_dcoef, const double *d_dh, int rows, int n_dirs, int order, int n_steps,
                           int lanes_per_row, void *d_out, qmle_stream stream_) {
  if (dim != 2 && dim != 4) return QMLE_ERR_UNSUPPORTED;
  if (order != 2 && order != 4) return QMLE_ERR_UNSUPPORTED;
  if (!h_terms || !d_coef || !d_h || !d_dcoef || !d_dh || !d_out || n_terms < 1 || n_terms > kEvolveMaxTerms ||
      rows < 1 || n_steps < 1 || n_dirs < 1 || n_dirs > 64)
    return QMLE_ERR_INVALID_ARG;
  if ((long long)n_steps * (order == 4 ? 2 : 1) * n_terms > (1ll << 31) - 1) return QMLE_ERR_INVALID_ARG;
  if (lanes_per_row != 0 && lanes_per_row != 1 && lanes_per_row != 4 && lanes_per_row != 16 && lanes_per_row != 64)
    return QMLE_ERR_INVALID_ARG;
  const int column_lanes = dim == 4 ? 4 : 1;  // a run's lanes: one per column of a 4x4 U
  if (lanes_per_row * column_lanes > kWave) return QMLE_ERR_INVALID_ARG;  // a unit's lanes share a wave
  const long long units = (long long)rows * n_dirs;
  int lanes = lanes_per_row;
  if (!lanes) {
    lanes = units <= (1ll << 30) ? evolve_auto_lanes((int)units, n_steps) : 1;
    if (lanes * column_lanes > kWave) lanes = kWave / column_lanes;
  }
  if (units * lanes > (1ll << 31) - kEvolveThreads) return QMLE_ERR_INVALID_ARG;
  EvolveTerms T;
  if (dim == 2) pack_terms<2>(h_terms, n_terms, T);
  else pack_terms<4>(h_terms, n_terms, T);
  for (int t = n_terms; t < kEvolveMaxTerms; ++t)
    for (int k = 0; k < 16; ++k) T.h[t][k] = 0.0;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(grid_for((uint64_t)(units * lanes * column_lanes), kEvolveThreads)), block(kEvolveThreads);
#define QMLE_EVOLVE_LAUNCH(D, O)                                                                                     \
  hipLaunchKernelGGL((k_evolve_magnus_jac<D, O>), grid, block, 0, stream, T, n_terms, d_coef, d_h, d_dcoef, d_dh, rows, \
                     n_dirs, n_steps, lanes, (double2 *)d_out)
  if (dim == 2 && order == 2) QMLE_EVOLVE_LAUNCH(2, 2);
  else if (dim == 2) QMLE_EVOLVE_LAUNCH(2, 4);
  else if (order == 2) QMLE_EVOLVE_LAUNCH(4, 2);
  else QMLE_EVOLVE_LAUNCH(4, 4);
#undef QMLE_EVOLVE_LAUNCH
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_pulse_unitaries(const double *d_solves, int n_solves, int envelope, int mode, double omega_c, double omega_q,
                         int order, int n_steps, int lanes_per_solve, int out_f64, void *d_out, const void *d_prev,
                         double *d_err, qmle_stream stream_) {
  PulseLaunch L{envelope, mode, n_solves, n_steps, 0, out_f64, omega_c, omega_q};
  dim3 grid;
  if (const int bad = pulse_launch(d_solves, d_out, order, lanes_per_solve, L, grid)) return bad;
  if ((out_f64 != 0 && out_f64 != 1) || (d_err && !d_prev)) return QMLE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_pulse(order, envelope, mode, [&](auto o, auto e, auto m) {
    hipLaunchKernelGGL((k_pulse_unitaries<o(), e(), m()>), grid, dim3(kEvolveThreads), 0, stream, d_solves, L, d_out,
                       d_prev, d_err);
  });
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_pulse_unitaries_jac(const double *d_solves, int n_solves, int envelope, int mode, double omega_c,
                             double omega_q, int order, int n_steps, int lanes_per_solve, void *d_out,
                             qmle_stream stream_) {
  PulseLaunch L{envelope, mode, n_solves, n_steps, 0, 1, omega_c, omega_q};
  dim3 grid;
  if (const int bad = pulse_launch(d_solves, d_out, order, lanes_per_solve, L, grid)) return bad;
  hipStream_t stream = (hipStream_t)stream_;
  dispatch_pulse(order, envelope, mode, [&](auto o, auto e, auto m) {
    hipLaunchKernelGGL((k_pulse_jac<o(), e(), m()>), grid, dim3(kEvolveThreads), 0, stream, d_solves, L,
                       (double2 *)d_out);
  });
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

size_t qmle_compose_workspace_bytes(int n_circuits, int n_ops, int n_terms, int64_t n_rows) {
  if (n_circuits < 1 || n_ops < 0 || n_terms < 0 || n_rows < 0) return 0;
  return align_up((size_t)n_circuits * sizeof(qmle_compose_circuit), 16) +
         align_up((size_t)n_ops * sizeof(qmle_compose_op), 16) + align_up((size_t)n_terms * sizeof(qmle_compose_term), 16) +
         align_up((size_t)n_rows * sizeof(int32_t), 16) + align_up((size_t)(n_circuits + 1) * sizeof(long long), 16);
}

int qmle_compose_circuits(const qmle_compose_circuit *circuits, int n_circuits, const qmle_compose_op *ops, int n_ops,
                          const qmle_compose_term *terms, int n_terms, const int32_t *rows, int64_t n_rows,
                          int n_candidates, const void *d_mats, int64_t n_mats, const double *d_coefs, int64_t n_coefs,
                          const void *d_targets, int64_t n_targets, const void *d_jac, int n_solves,
                          unsigned column_mask, void *d_ov, int64_t ov_len, void *d_full, int64_t full_len,
                          void *d_workspace, size_t workspace_bytes, qmle_stream stream_) {
  // every index a lane dereferences is checked here, against the table or pool it points into
  if (!circuits || n_circuits < 1 || n_candidates < 1 || n_ops < 0 || n_terms < 0 || n_rows < 0 || (n_ops && !ops) ||
      (n_terms && !terms) || (n_rows && !rows) || n_mats < 0 || n_coefs < 0 || n_targets < 0 || n_solves < 0 ||
      ov_len < 0 || full_len < 0 || (!d_ov && !d_full) || !(column_mask & 0xfu))
    return QMLE_ERR_INVALID_ARG;
  const long long C = n_candidates;
  constexpr long long kMaxParams = 1 << 20;
  // [off, off + len) inside a pool of n elements
  auto inside = [](long long off, long long len, long long n) { return off >= 0 && len >= 0 && off <= n && len <= n - off; };
  for (int64_t r = 0; r < n_rows; ++r)
    if (rows[r] < 0 || rows[r] >= n_solves) return QMLE_ERR_INVALID_ARG;
  for (int i = 0; i < n_ops; ++i) {
    const qmle_compose_op &o = ops[i];
    if (o.kind < QMLE_COMPOSE_CONST || o.kind > QMLE_COMPOSE_CPHASE || o.placement < 0 || o.placement > 4)
      return QMLE_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < n_ops; ++i) {
    const qmle_compose_op &o = ops[i];
    const bool wide = o.placement >= 3;
    const bool pulse = o.kind == QMLE_COMPOSE_PULSE;
    if ((pulse || (o.kind >= QMLE_COMPOSE_ROT_X && o.kind <= QMLE_COMPOSE_ROT_Z)) && wide) return QMLE_ERR_INVALID_ARG;
    if (o.kind == QMLE_COMPOSE_CPHASE && !wide) return QMLE_ERR_INVALID_ARG;
    if (pulse) {
      if (!d_jac || !inside(o.mat_off, C, n_rows)) return QMLE_ERR_INVALID_ARG;
    } else {
      const long long size = wide ? 16 : 4;
      if (!d_mats || o.mat_stride < 0 || (o.mat_stride > 0 && C - 1 > n_mats / o.mat_stride) || !inside(o.mat_off, (C - 1) * o.mat_stride + size, n_mats))
        return QMLE_ERR_INVALID_ARG;
    }
    if (!inside(o.term_begin, (long long)o.term_end - o.term_begin, n_terms)) return QMLE_ERR_INVALID_ARG;
    if (o.kind == QMLE_COMPOSE_CONST && o.term_end != o.term_begin) return QMLE_ERR_INVALID_ARG;
    for (int t = o.term_begin; t < o.term_end; ++t) {
      const qmle_compose_term &T = terms[t];
      if (T.slot < 0 || T.slot > (pulse ? 4 : 0) || T.param < 0 || !d_coefs || !inside(T.coef_off, C, n_coefs))
        return QMLE_ERR_INVALID_ARG;
    }
  }
  std::vector<long long> lane_begin((size_t)n_circuits + 1);
  std::vector<std::pair<long long, long long>> ov_ranges, full_ranges;  // [begin, end) of every output block
  long long lanes = 0;
  for (int k = 0; k < n_circuits; ++k) {
    const qmle_compose_circuit &K = circuits[k];
    if (K.n_wires != 1 && K.n_wires != 2) return QMLE_ERR_UNSUPPORTED;
    const long long d = 1ll << K.n_wires, P = K.n_params;
    if (P < 0 || P > kMaxParams || !inside(K.op_begin, (long long)K.op_end - K.op_begin, n_ops)) return QMLE_ERR_INVALID_ARG;
    if (K.target_off != -1 && (!d_targets || !inside(K.target_off, d * d, n_targets))) return QMLE_ERR_INVALID_ARG;
    if (d_ov && K.target_off != -1) {
      if (!inside(K.ov_off, C, ov_len) || !inside(K.dov_off, C * P, ov_len)) return QMLE_ERR_INVALID_ARG;
      if (!(column_mask & ((1u << d) - 1u))) return QMLE_ERR_INVALID_ARG;  // no column of this circuit selected
      ov_ranges.emplace_back(K.ov_off, K.ov_off + C);
      if (P) ov_ranges.emplace_back(K.dov_off, K.dov_off + C * P);
    }
    if (d_full) {
      if (!inside(K.u_off, C * d * d, full_len) || !inside(K.du_off, C * P * d * d, full_len)) return QMLE_ERR_INVALID_ARG;
      full_ranges.emplace_back(K.u_off, K.u_off + C * d * d);
      if (P) full_ranges.emplace_back(K.du_off, K.du_off + C * P * d * d);
    }
    for (int i = K.op_begin; i < K.op_end; ++i) {
      const qmle_compose_op &o = ops[i];
      if ((o.placement == 0) != (K.n_wires == 1)) return QMLE_ERR_INVALID_ARG;
      for (int t = o.term_begin; t < o.term_end; ++t)
        if (terms[t].param >= P) return QMLE_ERR_INVALID_ARG;
    }
    lane_begin[k] = lanes;
    lanes += align_up((size_t)(C * (P + 1) * d), 4);
    if (lanes > (1ll << 31) - kEvolveThreads) return QMLE_ERR_INVALID_ARG;  // grid.x
  }
  lane_begin[n_circuits] = lanes;
  for (auto *ranges : {&ov_ranges, &full_ranges}) {  // two lanes must never store to one element
    std::sort(ranges->begin(), ranges->end());
    for (size_t i = 1; i < ranges->size(); ++i)
      if ((*ranges)[i].first < (*ranges)[i - 1].second) return QMLE_ERR_INVALID_ARG;
  }
  const size_t need = qmle_compose_workspace_bytes(n_circuits, n_ops, n_terms, n_rows);
  if (!d_workspace || workspace_bytes < need || ((uintptr_t)d_workspace & 15u)) return QMLE_ERR_WORKSPACE;

  // the tables travel as asynchronous copies from pageable memory, which the runtime stages before the copy call
  // returns (as the term tables of the Pauli entry points; the header states what that asks of the caller)
  hipStream_t stream = (hipStream_t)stream_;
  char *at = (char *)d_workspace;
  auto upload = [&](const void *src, size_t bytes, const void **dst) -> hipError_t {
    *dst = at;
    at += align_up(bytes, 16);
    return bytes ? hipMemcpyAsync((void *)*dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess;
  };
  ComposeLaunch L{};
  HIPCHK(upload(circuits, (size_t)n_circuits * sizeof(qmle_compose_circuit), (const void **)&L.circuits));
  HIPCHK(upload(ops, (size_t)n_ops * sizeof(qmle_compose_op), (const void **)&L.ops));
  HIPCHK(upload(terms, (size_t)n_terms * sizeof(qmle_compose_term), (const void **)&L.terms));
  HIPCHK(upload(rows, (size_t)n_rows * sizeof(int32_t), (const void **)&L.rows));
  HIPCHK(upload(lane_begin.data(), lane_begin.size() * sizeof(long long), (const void **)&L.lane_begin));
  L.mats = (const double2 *)d_mats;
  L.coefs = d_coefs;
  L.targets = (const double2 *)d_targets;
  L.jac = (const double2 *)d_jac;
  L.ov = (double2 *)d_ov;
  L.full = (double2 *)d_full;
  L.n_circuits = n_circuits;
  L.n_candidates = n_candidates;
  L.column_mask = column_mask;
  hipLaunchKernelGGL(k_compose_circuits, dim3(grid_for((uint64_t)lanes, kEvolveThreads)), dim3(kEvolveThreads), 0, stream,
                     L);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

}  // extern "C"
