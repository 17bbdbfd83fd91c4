// Per-sample gate matrices from the angle table (templates shared by the complex64 engine and the
// complex128 one): operations.py:1002-1045, 1053-1100, 1171-1243, 1255-1351, 1357-1487 restated.
#pragma once
#include "qmle_dev.h"

namespace {

// ---------------------------------------------------------------------------
// per-sample gate matrices  (operations.py:1002-1045, 1053-1100, 1171-1243,
// 1255-1351, 1357-1487 -- matrices restated, evaluated in fp64, stored fp32)
// ---------------------------------------------------------------------------
struct cd {
  double re, im;
};
__host__ __device__ __forceinline__ cd cdmul(cd a, cd b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

__host__ __device__ __forceinline__ cd cdadd(cd a, cd b) { return {a.re + b.re, a.im + b.im}; }
__host__ __device__ __forceinline__ cd cddiv(cd a, cd b) {
  const double d = b.re * b.re + b.im * b.im;
  return {(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
struct M2 {
  cd a, b, c, d;  // [[a, b], [c, d]]
};

// ---------------------------------------------------------------------------
// unit-pivot form (k_tile2's FC_UDENSE / FC_UDIAG): U = pivot * U' with a literal 1 in U', so that the gate costs 6
// packed instructions per amplitude pair instead of 8; the pivots of a chain are multiplied into P and handed to the
// chain's last member, the carrier, which is stored as P U in the plain layout (a scalar commutes with every gate in
// between).  One member of a chain: writes its 8-float record to `out`, updates P, returns the pivot it divided by.
//   CM_UNIT_DENSE  pivot = m00 if |m00| >= |m01| (form 1: [[1, x], [y, z]]), else m01 (form 2: [[x, 1], [y, z]]);
//                  record {x, y, z, (form, 0)} -- the form word is the float 1 or 2.  A unitary 2x2 has
//                  |m00|^2 + |m01|^2 = 1, so |pivot| >= 1 / sqrt 2 and m00 = 0 (RY(pi)) is form 2
//   CM_UNIT_DIAG   pivot = m00 (modulus 1): record diag(1, m11 / m00) in the plain layout
//   CM_CARRIER     record P U in the plain layout; P starts again at 1
// ---------------------------------------------------------------------------
template <class OT>
__host__ __device__ __forceinline__ cd unit_chain_step(const M2 &U, int member, cd &P, OT *out) {
  if (member == CM_CARRIER) {
    const cd a = cdmul(P, U.a), b = cdmul(P, U.b), c = cdmul(P, U.c), d = cdmul(P, U.d);
    out[0] = (OT)a.re; out[1] = (OT)a.im; out[2] = (OT)b.re; out[3] = (OT)b.im;
    out[4] = (OT)c.re; out[5] = (OT)c.im; out[6] = (OT)d.re; out[7] = (OT)d.im;
    P = {1.0, 0.0};
    return {1.0, 0.0};
  }
  if (member == CM_UNIT_DIAG) {
    const cd piv = U.a, w = cddiv(U.d, piv);
    out[0] = (OT)1; out[1] = (OT)0; out[2] = (OT)0; out[3] = (OT)0;
    out[4] = (OT)0; out[5] = (OT)0; out[6] = (OT)w.re; out[7] = (OT)w.im;
    P = cdmul(P, piv);
    return piv;
  }
  const bool form1 = U.a.re * U.a.re + U.a.im * U.a.im >= U.b.re * U.b.re + U.b.im * U.b.im;
  const cd piv = form1 ? U.a : U.b;
  const cd x = cddiv(form1 ? U.b : U.a, piv), y = cddiv(U.c, piv), z = cddiv(U.d, piv);
  out[0] = (OT)x.re; out[1] = (OT)x.im; out[2] = (OT)y.re; out[3] = (OT)y.im;
  out[4] = (OT)z.re; out[5] = (OT)z.im; out[6] = (OT)(form1 ? 1 : 2); out[7] = (OT)0;
  P = cdmul(P, piv);
  return piv;
}
// the operator a chain member's ops2 record applies: U / pivot (unit forms; the pivot enters P), P U (the carrier; P
// starts again at 1), U (CM_PLAIN) -- the arithmetic of unit_chain_step, without the record
__host__ __device__ __forceinline__ M2 unit_chain_operator(const M2 &U, int member, cd &P) {
  if (member == CM_CARRIER) {
    const M2 R = {cdmul(P, U.a), cdmul(P, U.b), cdmul(P, U.c), cdmul(P, U.d)};
    P = {1.0, 0.0};
    return R;
  }
  if (member == CM_PLAIN) return U;
  cd piv = U.a;
  if (member == CM_UNIT_DENSE && !(U.a.re * U.a.re + U.a.im * U.a.im >= U.b.re * U.b.re + U.b.im * U.b.im)) piv = U.b;
  P = cdmul(P, piv);
  return {cddiv(U.a, piv), cddiv(U.b, piv), cddiv(U.c, piv), cddiv(U.d, piv)};
}

// ---------------------------------------------------------------------------
// product form of a group (k_tile2's product_group).  A 2x2 matrix that is a scalar times a unitary is
//   M = g diag(1, l) [[c, -s], [s, c]] diag(1, r),   c = |m00| / |g|, s = |m10| / |g| >= 0, |g|^2 = |m00|^2 + |m10|^2,
// l, r and g / |g| unit phases (moduli and divisions only).  Where s = 0 the phase is split as r = 1, l = m11 / g;
// where c = 0 as l = 1, g = m10 / s.  The real middle step runs without its scale:
//   c >= s (form 1, direct)    t = s / c:  a0 -= t a1;  a1 += u a0,  u = t / (1 + t^2)  -- leaves
//                              diag(1, 1 / (1 + t^2)) [[1, -t], [t, 1]] (a0, a1); the record holds (-t, u) and the
//                              closing factors are g c and g l c (1 + t^2)
//   c <  s (form 2, mirrored)  t' = c / s: [[t', -1], [1, t']]; the record holds (t', 0), closing factors g s and g l s
// Over the n <= 4 members of a group, on distinct in-thread bits: opening entry e = product of r_q over the members
// whose bit is set in e, closing entry e = product of the members' factor for their bit of e.  fp64 throughout, rounded
// once on the store; layout: kProductRec* (qmle_internal.h).  forms (optional): the form of each member.
// measured: the record of a run in which only basis permutations and |amplitude|^2 follow the group.  The
// phases g / |g| and l are then invisible, and the rotation is applied exactly, as three shears that need no scale:
//   [[c, -s], [s, c]] = [[1, -tau], [0, 1]] [[1, 0], [s, 1]] [[1, -tau], [0, 1]],  tau = s / (1 + c) <= 1   (form 3)
// -- a0 -= tau a1; a1 += s a0; a0 -= tau a1; the record holds (-tau, s).  No mirrored case, the closing entries are
// exact ones, and the word kProductRecNoClose tells the kernel to leave them out.  What such a record applies is
// D (x)_q M_q / |g_q| for a diagonal D of unit phases: |g_q| is dropped too (1 for a unitary; the pivots of a
// unit-pivot chain cancel over the chain's members, which is why a chain is measured as a whole or not at all).
// ---------------------------------------------------------------------------
template <class OT>
__host__ __device__ inline void product_form_group(const M2 *m, const int *bit, int n, OT *out, int *forms = nullptr,
                                                   bool measured = false) {
  cd open[16], close[16];
  for (int e = 0; e < 16; ++e) open[e] = close[e] = {1.0, 0.0};
  for (uint32_t i = kProductRecSteps; i < kProductRecClose; ++i) out[i] = (OT)0;
  if (measured) out[kProductRecNoClose] = (OT)1;
  for (int q = 0; q < n; ++q) {
    const M2 &M = m[q];
    const double n00 = M.a.re * M.a.re + M.a.im * M.a.im, n10 = M.c.re * M.c.re + M.c.im * M.c.im;
    const double N = sqrt(n00 + n10), c = sqrt(n00) / N, s = sqrt(n10) / N;
    const bool direct = c >= s;
    cd g, l, r;
    if (direct) {
      g = {M.a.re / c, M.a.im / c};
      if (s > 0.0) {
        const cd gs = {g.re * s, g.im * s};
        l = cddiv(M.c, gs);
        r = cddiv({-M.b.re, -M.b.im}, gs);
      } else {
        l = cddiv(M.d, g);
        r = {1.0, 0.0};
      }
    } else {
      const cd h = {M.c.re / s, M.c.im / s};  // g l
      if (c > 0.0) {
        g = {M.a.re / c, M.a.im / c};
        l = cddiv(h, g);
      } else {
        g = h;
        l = {1.0, 0.0};
      }
      r = cddiv({-M.b.re, -M.b.im}, {g.re * s, g.im * s});
    }
    const cd gl = cdmul(g, l);
    cd lo, hi;
    double w0, w1;
    int form = direct ? 1 : 2;
    if (measured) {
      w0 = -s / (1.0 + c);
      w1 = s;
      lo = hi = {1.0, 0.0};
      form = 3;
    } else if (direct) {
      const double t = s / c;
      w0 = -t;
      w1 = t / (1.0 + t * t);
      lo = {g.re * c, g.im * c};
      hi = {gl.re * (c * (1.0 + t * t)), gl.im * (c * (1.0 + t * t))};
    } else {
      w0 = c / s;
      w1 = 0.0;
      lo = {g.re * s, g.im * s};
      hi = {gl.re * s, gl.im * s};
    }
    const int b = bit[q];
    out[kProductRecSteps + 2 * b] = (OT)w0;
    out[kProductRecSteps + 2 * b + 1] = (OT)w1;
    out[kProductRecForms + b] = (OT)form;
    if (forms) forms[q] = form;
    for (int e = 0; e < 16; ++e) {
      if ((e >> b) & 1) {
        open[e] = cdmul(open[e], r);
        close[e] = cdmul(close[e], hi);
      } else {
        close[e] = cdmul(close[e], lo);
      }
    }
  }
  for (int e = 0; e < 16; ++e) {
    out[2 * e] = (OT)open[e].re;
    out[2 * e + 1] = (OT)open[e].im;
    out[kProductRecClose + 2 * e] = (OT)close[e].re;
    out[kProductRecClose + 2 * e + 1] = (OT)close[e].im;
  }
}

// the 2x2 source gates of source_matrix(), entries in registers
// ANG: anything indexable by slot -- a row of the angle table (`const float *` / `const double *`) or an
// AngleMapRow that forms the angle from the leaves on the fly (same arithmetic as k_build_angles)
template <class ANG, class CT>
__device__ __forceinline__ M2 source_2x2(const BuildOp &b, ANG ang, const CT *__restrict__ consts) {
  const cd z = {0.0, 0.0}, one = {1.0, 0.0};
  // (ahead of the switch, not an arm of it: with this source as one more arm, hipcc 7 built CRX / CRZ / CPhase
  // matrices that were wrong by 0.6 in the state -- tests/test_gpu_evolution.py keeps a circuit with all of them)
  if (b.opcode == QMLE_OP_MAT1_ROW) {  // the sample's own 2x2: 8 consecutive columns of its table row
    const int s0 = b.slot[0];
    return {{(double)ang[s0 + 0], (double)ang[s0 + 1]}, {(double)ang[s0 + 2], (double)ang[s0 + 3]},
            {(double)ang[s0 + 4], (double)ang[s0 + 5]}, {(double)ang[s0 + 6], (double)ang[s0 + 7]}};
  }
  double th = 0.0, c = 1.0, s = 0.0;
  if (b.slot[0] >= 0) {
    th = (double)ang[b.slot[0]];
    sincos(0.5 * th, &s, &c);
  }
  const double r2 = 0.70710678118654752440;
  switch (b.opcode) {
    case QMLE_OP_X: case QMLE_OP_CX: case QMLE_OP_CCX: return {z, one, one, z};
    case QMLE_OP_Y: case QMLE_OP_CY: return {z, {0, -1}, {0, 1}, z};
    case QMLE_OP_Z: case QMLE_OP_CZ: return {one, z, z, {-1, 0}};
    case QMLE_OP_H: return {{r2, 0}, {r2, 0}, {r2, 0}, {-r2, 0}};
    case QMLE_OP_S: return {one, z, z, {0, 1}};
    case QMLE_OP_RX: case QMLE_OP_CRX: return {{c, 0}, {0, -s}, {0, -s}, {c, 0}};
    case QMLE_OP_RY: case QMLE_OP_CRY: return {{c, 0}, {-s, 0}, {s, 0}, {c, 0}};
    case QMLE_OP_RZ: case QMLE_OP_CRZ: return {{c, -s}, z, z, {c, s}};
    case QMLE_OP_CPHASE: {
      double sp, cp;
      sincos(th, &sp, &cp);
      return {one, z, z, {cp, sp}};
    }
    case QMLE_OP_ROT: {  // RZ(omega) RY(theta) RZ(phi), operations.py:1234-1243
      const double phi = (double)ang[b.slot[0]], theta = (double)ang[b.slot[1]], omega = (double)ang[b.slot[2]];
      double st, ct, sp, cp, sm, cm;
      sincos(0.5 * theta, &st, &ct);
      sincos(0.5 * (phi + omega), &sp, &cp);
      sincos(0.5 * (phi - omega), &sm, &cm);
      return {{cp * ct, -sp * ct}, {-cm * st, -sm * st}, {cm * st, -sm * st}, {cp * ct, sp * ct}};
    }
    case QMLE_OP_MAT1:
      return {{(double)consts[b.const_off + 0], (double)consts[b.const_off + 1]},
              {(double)consts[b.const_off + 2], (double)consts[b.const_off + 3]},
              {(double)consts[b.const_off + 4], (double)consts[b.const_off + 5]},
              {(double)consts[b.const_off + 6], (double)consts[b.const_off + 7]}};
    default: return {one, z, z, one};
  }
}

template <class ANG, class CT>
__device__ void source_matrix(const BuildOp &b, ANG ang,
                              const CT *__restrict__ consts, cd *M, int dim) {
  const int nn = dim * dim;
  for (int i = 0; i < nn; ++i) M[i] = {0.0, 0.0};
  if (b.opcode == QMLE_OP_MAT1_ROW || b.opcode == QMLE_OP_MAT2_ROW) {  // the sample's own matrix
    for (int i = 0; i < nn; ++i) M[i] = {(double)ang[b.slot[0] + 2 * i], (double)ang[b.slot[0] + 2 * i + 1]};
    return;
  }
  double th = 0.0, c = 1.0, s = 0.0;
  if (b.slot[0] >= 0) {
    th = (double)ang[b.slot[0]];
    sincos(0.5 * th, &s, &c);
  }
  const double r2 = 0.70710678118654752440;
  switch (b.opcode) {
    case QMLE_OP_X: case QMLE_OP_CX: case QMLE_OP_CCX:
      M[1] = {1, 0}; M[2] = {1, 0}; break;
    case QMLE_OP_Y: case QMLE_OP_CY:
      M[1] = {0, -1}; M[2] = {0, 1}; break;
    case QMLE_OP_Z: case QMLE_OP_CZ:
      M[0] = {1, 0}; M[3] = {-1, 0}; break;
    case QMLE_OP_H:
      M[0] = {r2, 0}; M[1] = {r2, 0}; M[2] = {r2, 0}; M[3] = {-r2, 0}; break;
    case QMLE_OP_S:
      M[0] = {1, 0}; M[3] = {0, 1}; break;
    case QMLE_OP_RX: case QMLE_OP_CRX:  // c I - i s X
      M[0] = {c, 0}; M[1] = {0, -s}; M[2] = {0, -s}; M[3] = {c, 0}; break;
    case QMLE_OP_RY: case QMLE_OP_CRY:  // c I - i s Y
      M[0] = {c, 0}; M[1] = {-s, 0}; M[2] = {s, 0}; M[3] = {c, 0}; break;
    case QMLE_OP_RZ: case QMLE_OP_CRZ:  // diag(c - i s, c + i s)
      M[0] = {c, -s}; M[3] = {c, s}; break;
    case QMLE_OP_CPHASE: {              // diag(1, e^{i phi}) on the target
      double sp, cp;
      sincos(th, &sp, &cp);
      M[0] = {1, 0}; M[3] = {cp, sp}; break;
    }
    case QMLE_OP_ROT: {  // RZ(omega) RY(theta) RZ(phi), operations.py:1234-1243
      const double phi = (double)ang[b.slot[0]], theta = (double)ang[b.slot[1]],
                   omega = (double)ang[b.slot[2]];
      double st, ct, sp, cp, sm, cm;
      sincos(0.5 * theta, &st, &ct);
      sincos(0.5 * (phi + omega), &sp, &cp);
      sincos(0.5 * (phi - omega), &sm, &cm);
      M[0] = {cp * ct, -sp * ct};
      M[1] = {-cm * st, -sm * st};
      M[2] = {cm * st, -sm * st};
      M[3] = {cp * ct, sp * ct};
      break;
    }
    case QMLE_OP_SWAP: case QMLE_OP_CSWAP:
      M[0] = {1, 0}; M[6] = {1, 0}; M[9] = {1, 0}; M[15] = {1, 0}; break;
    case QMLE_OP_RXX:  // c I - i s X(x)X : anti-diagonal
      for (int i = 0; i < 4; ++i) { M[i * 4 + i] = {c, 0}; M[i * 4 + (3 - i)] = {0, -s}; }
      break;
    case QMLE_OP_RYY:  // Y(x)Y = antidiag(-1, 1, 1, -1)
      for (int i = 0; i < 4; ++i) {
        M[i * 4 + i] = {c, 0};
        const double sg = (i == 0 || i == 3) ? -1.0 : 1.0;
        M[i * 4 + (3 - i)] = {0, -s * sg};
      }
      break;
    case QMLE_OP_RZZ:  // diag(e^{-i t/2}, e^{+}, e^{+}, e^{-})
      M[0] = {c, -s}; M[5] = {c, s}; M[10] = {c, s}; M[15] = {c, -s}; break;
    case QMLE_OP_RZX:  // Z(x)X = [[X,0],[0,-X]]
      for (int i = 0; i < 4; ++i) M[i * 4 + i] = {c, 0};
      M[1] = {0, -s}; M[4] = {0, -s}; M[11] = {0, s}; M[14] = {0, s};
      break;
    case QMLE_OP_MAT1: case QMLE_OP_MAT2:
      for (int i = 0; i < nn; ++i)
        M[i] = {(double)consts[b.const_off + 2 * i], (double)consts[b.const_off + 2 * i + 1]};
      break;
    default:  // identity
      for (int i = 0; i < dim; ++i) M[i * dim + i] = {1, 0};
      break;
  }
}

// Angle table computed on the fly: table[b][s] = c[s] + sum_t coef[t] * leaf_{arg[t]}[row_k(b)][idx[t]],
// row_k(b) = ((b + b_offset) / div_k) % mod_k, fp64 sum, reduced into [-period/2, period/2] where it lies beyond
// +-period (and only there), rounded to float32 -- bit for bit what k_build_angles stores (qmle_engine.hip); qmle_run_batch_map uses it to skip
// that kernel and the table's round trip when nothing but the matrix builder reads angles.
struct AngleLeaves {
  const float *ptr[8];
  long long stride[8];  // floats per row
  int div[8], mod[8];
};
struct AngleMapSrc {
  AngleLeaves lv;
  const int *ptr, *arg, *idx;
  const float *coef, *cst;
  const double *period;
  long long b_offset;
  int small;  // batch + offset < 2^32: row arithmetic in 32 bits
};
struct AngleMapRow {
  const AngleMapSrc *m;
  unsigned long long gb;
  __device__ __forceinline__ float operator[](int s) const {
    double acc = (double)m->cst[s];
    for (int t = m->ptr[s]; t < m->ptr[s + 1]; ++t) {
      const int k = m->arg[t];
      const long long row = m->small ? (long long)(((uint32_t)gb / (uint32_t)m->lv.div[k]) % (uint32_t)m->lv.mod[k])
                                     : (long long)((gb / (unsigned long long)m->lv.div[k]) % (unsigned long long)m->lv.mod[k]);
      acc = fma((double)m->coef[t], (double)m->lv.ptr[k][row * m->lv.stride[k] + m->idx[t]], acc);
    }
    const double per = m->period ? m->period[s] : 0.0;
    if (per > 0.0 && (acc > per || acc < -per)) acc -= per * rint(acc / per);
    return (float)acc;
  }
};
template <class T>
__device__ __forceinline__ const T *angle_row(const T *table, int b, int n_slots) { return table + (size_t)b * n_slots; }
__device__ __forceinline__ AngleMapRow angle_row(const AngleMapSrc &m, int b, int) {
  return AngleMapRow{&m, (unsigned long long)((long long)b + m.b_offset)};
}

// AT / CT / OT: angle table, constant blob and matrix row types -- float / float / float for the
// complex64 engine, double throughout for the complex128 one (qmle_run_batch_f64)
// GMAJOR: whole waves per group (launch side: batch >= 64, blocks of one wave) -- the group index is then
// provably wave-uniform and the descriptors come through the scalar cache
// ASRC: `const AT *` (the angle table) or `const AngleMapSrc &`
// PRODUCT: the launch builds the product-form records of the fast groups (BuildGroup::dim = kBuildProduct, the
// n_product_groups last needed items) and nothing else; every other launch leaves those items out -- a kernel of their
// own, so that the 32 fp64 complex numbers of the two diagonals do not set the register count of the common builder
// measured_from (PRODUCT): records at this float offset of the row and behind it -- the last stage's, in a run that
// ends in |amplitude|^2 only -- are built in measured mode where their group allows it (the markers' pad2);
// kNoMeasuredRecords: none, every record is phase-exact
constexpr uint32_t kNoMeasuredRecords = 0xffffffffu;
template <class ASRC, class CT, class OT, bool GMAJOR = false, bool PRODUCT = false>
__device__ __forceinline__ void build_matrices_body(const BuildOp *__restrict__ build,
                                                    const BuildGroup *__restrict__ groups, int n_groups,
                                                    ASRC angles, int n_slots,
                                                    const CT *__restrict__ consts, OT *__restrict__ mats,
                                                    uint32_t mat_floats, int batch,
                                                    uint32_t measured_from = kNoMeasuredRecords) {
  // one work item per (sample, group).  batch >= 64 (blocks of ONE wave): a wave takes 64 consecutive
  // samples of the SAME group -- every lane then walks the same source gates through the same branches
  // of the opcode switch.  With the samples-then-groups flattening used below that, neighbouring lanes
  // held different groups (RX next to RY next to CX ...) and a wave executed every branch any of its lanes
  // needed, one after the other: 20 us for the 4096 x 130 groups of the Fourier grid, untouched by cheaper
  // trigonometry, fewer registers, prefetched descriptors or LDS staging.
  int b, g;
  if constexpr (GMAJOR) {
    const uint32_t per = ((uint32_t)batch + 63u) >> 6;  // waves per group
    g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / per));
    b = (int)((blockIdx.x - (uint32_t)g * per) * 64u + threadIdx.x);
    if (g >= n_groups || b >= batch) return;
  } else {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long b_ll = idx / n_groups;
    if (b_ll >= batch) return;
    b = (int)b_ll;
    g = (int)(idx - b_ll * n_groups);
  }
  const BuildGroup grp = groups[g];
  const auto ang = angle_row(angles, b, n_slots);
  const int dim = (int)grp.dim;
  if (grp.dim == kBuildChain) {
    // one work item per (sample, chain): the members' fused 2x2 in stream order, each closed by its marker
    // (the walk is the same for every sample: under GMAJOR a wave diverges on the form of a pivot only)
    cd P = {1.0, 0.0};
    M2 M = {{1.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {1.0, 0.0}};
    bool first = true;
    for (uint32_t k = grp.begin; k < grp.end; ++k) {
      const BuildOp bo = build[k];
      if (bo.opcode == kChainMark) {
        (void)unit_chain_step(M, (int)bo.pad, P, mats + (size_t)b * mat_floats + (uint32_t)bo.const_off);
        first = true;
        continue;
      }
      const M2 S = source_2x2(bo, ang, consts);  // later gate on the left: M <- S M
      if (first) {
        M = S;
        first = false;
        continue;
      }
      const cd a = cdadd(cdmul(S.a, M.a), cdmul(S.b, M.c)), bb = cdadd(cdmul(S.a, M.b), cdmul(S.b, M.d));
      const cd c = cdadd(cdmul(S.c, M.a), cdmul(S.d, M.c)), d = cdadd(cdmul(S.c, M.b), cdmul(S.d, M.d));
      M = {a, bb, c, d};
    }
    return;
  }
  if ((grp.dim == kBuildProduct) != PRODUCT) return;
  if constexpr (PRODUCT) {
    // one work item per (sample, product-form group): the members' fused 2x2 in stream order, turned into the operator
    // their ops2 record applies (the chain's P walks along), then the group's record
    cd P = {1.0, 0.0};
    M2 M = {{1.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {1.0, 0.0}}, mem[4];
    int bit[4], n_mem = 0;
    bool first = true, closing_free = false;
    for (uint32_t k = grp.begin; k < grp.end; ++k) {
      const BuildOp bo = build[k];
      if (bo.opcode == kChainMark) {
        closing_free = bo.pad2 != 0;
        const M2 E = unit_chain_operator(M, (int)bo.pad, P);
        if (bo.const_off >= 0 && n_mem < 4) {
          mem[n_mem] = E;
          bit[n_mem++] = bo.const_off;
        }
        first = true;
        continue;
      }
      const M2 S = source_2x2(bo, ang, consts);  // later gate on the left: M <- S M
      if (first) {
        M = S;
        first = false;
        continue;
      }
      const cd a = cdadd(cdmul(S.a, M.a), cdmul(S.b, M.c)), bb = cdadd(cdmul(S.a, M.b), cdmul(S.b, M.d));
      const cd c = cdadd(cdmul(S.c, M.a), cdmul(S.d, M.c)), d = cdadd(cdmul(S.c, M.b), cdmul(S.d, M.d));
      M = {a, bb, c, d};
    }
    product_form_group(mem, bit, n_mem, mats + (size_t)b * mat_floats + grp.mat_off, nullptr,
                       closing_free && grp.mat_off >= measured_from);
    return;
  }
  if (dim == 2) {
    // 2x2 groups (all but the two-qubit Pauli rotations / SWAP / explicit 4x4): four named
    // entries in registers -- the generic path below indexes its arrays at run time and lives in
    // scratch, which made this kernel a third of the GPU time of the LDS-resident regime
    // (C4: 0.37 of 1.1 ms per 65536 states; profiles/r03_lds_regime_anatomy.txt)
    M2 M = source_2x2(build[grp.begin], ang, consts);
    for (uint32_t k = grp.begin + 1; k < grp.end; ++k) {
      const M2 S = source_2x2(build[k], ang, consts);  // later gate on the left: M <- S M
      const cd a = cdadd(cdmul(S.a, M.a), cdmul(S.b, M.c)), bb = cdadd(cdmul(S.a, M.b), cdmul(S.b, M.d));
      const cd c = cdadd(cdmul(S.c, M.a), cdmul(S.d, M.c)), d = cdadd(cdmul(S.c, M.b), cdmul(S.d, M.d));
      M = {a, bb, c, d};
    }
    OT *out = mats + (size_t)b * mat_floats + grp.mat_off;
    out[0] = (OT)M.a.re; out[1] = (OT)M.a.im; out[2] = (OT)M.b.re; out[3] = (OT)M.b.im;
    out[4] = (OT)M.c.re; out[5] = (OT)M.c.im; out[6] = (OT)M.d.re; out[7] = (OT)M.d.im;
    return;
  }
  cd M[16], S[16], R[16];
  // (BuildOp::pad = 1 / 2: a 2x2 source on the first / second wire of the pair, U (x) I / I (x) U -- row = 2 * bit[t0] + bit[t1])
  auto source4 = [&](const BuildOp &bo, cd *X) {
    if (dim != 4 || bo.pad == 0) {
      source_matrix(bo, ang, consts, X, dim);
      return;
    }
    const M2 U = source_2x2(bo, ang, consts);
    for (int i = 0; i < 16; ++i) X[i] = {0.0, 0.0};
    if (bo.pad == 1) {
      X[0] = U.a; X[2] = U.b; X[5] = U.a; X[7] = U.b; X[8] = U.c; X[10] = U.d; X[13] = U.c; X[15] = U.d;
    } else {
      X[0] = U.a; X[1] = U.b; X[4] = U.c; X[5] = U.d; X[10] = U.a; X[11] = U.b; X[14] = U.c; X[15] = U.d;
    }
  };
  source4(build[grp.begin], M);
  for (uint32_t k = grp.begin + 1; k < grp.end; ++k) {
    source4(build[k], S);
    for (int r = 0; r < dim; ++r)
      for (int c = 0; c < dim; ++c) {
        cd acc = {0, 0};
        for (int x = 0; x < dim; ++x) {
          const cd t = cdmul(S[r * dim + x], M[x * dim + c]);
          acc.re += t.re;
          acc.im += t.im;
        }
        R[r * dim + c] = acc;
      }
    for (int i = 0; i < dim * dim; ++i) M[i] = R[i];
  }
  OT *out = mats + (size_t)b * mat_floats + grp.mat_off;
  for (int i = 0; i < dim * dim; ++i) {
    out[2 * i] = (OT)M[i].re;
    out[2 * i + 1] = (OT)M[i].im;
  }
}

}  // namespace
