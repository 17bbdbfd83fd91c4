// libqmle_sv, engine: plan objects on the device, the angle table / gate matrix builders, and the
// C-ABI entry points that run a plan (qmle_run_batch, qmle_apply_inplace, profiling).
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
#include "qmle_matrices.h"

#include <map>
#include <mutex>
#include <vector>

namespace {

template <bool GMAJOR>
__global__ void __launch_bounds__(64)
k_build_matrices(const BuildOp *__restrict__ build, const BuildGroup *__restrict__ groups, int n_groups,
                 const float *__restrict__ angles, int n_slots, const float *__restrict__ consts,
                 float *__restrict__ mats, uint32_t mat_floats, int batch) {
  build_matrices_body<const float *, float, float, GMAJOR>(build, groups, n_groups, angles, n_slots, consts, mats, mat_floats, batch);
}

// the same straight from the affine angle map (qmle_run_batch_map; whole waves per group only)
__global__ void __launch_bounds__(64)
k_build_matrices_map(const BuildOp *__restrict__ build, const BuildGroup *__restrict__ groups, int n_groups,
                     const AngleMapSrc map, int n_slots, const float *__restrict__ consts,
                     float *__restrict__ mats, uint32_t mat_floats, int batch) {
  build_matrices_body<const AngleMapSrc &, float, float, true>(build, groups, n_groups, map, n_slots, consts, mats,
                                                              mat_floats, batch);
}

// the product-form records of the fast groups (build_matrices_body<.., PRODUCT>): `groups` = those items only
template <bool GMAJOR>
__global__ void __launch_bounds__(64)
k_build_matrices_product(const BuildOp *__restrict__ build, const BuildGroup *__restrict__ groups, int n_groups,
                const float *__restrict__ angles, int n_slots, const float *__restrict__ consts,
                float *__restrict__ mats, uint32_t mat_floats, int batch, uint32_t measured_from) {
  build_matrices_body<const float *, float, float, GMAJOR, true>(build, groups, n_groups, angles, n_slots, consts, mats, mat_floats, batch,
                                                                 measured_from);
}
__global__ void __launch_bounds__(64)
k_build_matrices_product_map(const BuildOp *__restrict__ build, const BuildGroup *__restrict__ groups, int n_groups,
                    const AngleMapSrc map, int n_slots, const float *__restrict__ consts,
                    float *__restrict__ mats, uint32_t mat_floats, int batch, uint32_t measured_from) {
  build_matrices_body<const AngleMapSrc &, float, float, true, true>(build, groups, n_groups, map, n_slots, consts, mats,
                                                                    mat_floats, batch, measured_from);
}

// ---------------------------------------------------------------------------
// angle table from device-resident leaves:  table[b][s] = c[s] + sum_t coef[t] * leaf_{arg[t]}[row][idx[t]]
// (gate angles are affine in params / inputs, ansaetze.py:323-371, model.py:804-816); the row
// of leaf k for flattened sample b is (b / div_k) % mod_k -- the cartesian batch of
// model.py:1449-1481 without materialising the repeats.
// ---------------------------------------------------------------------------
// One work item per (state, slot), flattened (every lane busy whatever the slot count: a block-per-state
// layout with the divisions hoisted out of the term loop measured 6.5 instead of 4.1 us for the 2048 x 108
// table of the Expressibility loop -- the kernel is a chain of three dependent loads, not arithmetic).
// IDX: 32-bit index arithmetic when batch x slots and batch + offset allow, 64-bit otherwise.
template <class IDX>
__global__ void __launch_bounds__(256)
k_build_angles(AngleLeaves lv, const int *__restrict__ ptr, const int *__restrict__ arg,
               const int *__restrict__ idx, const float *__restrict__ coef,
               const float *__restrict__ cst, const double *__restrict__ period, int n_slots,
               long long batch, long long b_offset, float *__restrict__ out) {
  const IDX i = (IDX)blockIdx.x * 256u + threadIdx.x;
  if ((long long)i >= batch * n_slots) return;
  const IDX b = i / (IDX)n_slots;
  const int s = (int)(i - b * (IDX)n_slots);
  const IDX gb = b + (IDX)b_offset;
  // fp64 accumulation; a sum beyond +-period is then reduced into [-period/2, period/2] (4 pi for a rotation
  // gate, which depends on angle / 2 only; a sum within +-period, the bounds included, stays as it is): binary /
  // ternary encodings scale inputs by up to 3^(n-1), and a float32 angle of ~1500 rad would carry 1e-4 rad of
  // rounding into the gate matrices
  double acc = (double)cst[s];
  for (int t = ptr[s]; t < ptr[s + 1]; ++t) {
    const int k = arg[t];
    const long long row = (long long)((gb / (IDX)lv.div[k]) % (IDX)lv.mod[k]);
    acc = fma((double)coef[t], (double)lv.ptr[k][row * lv.stride[k] + idx[t]], acc);
  }
  const double per = period ? period[s] : 0.0;
  if (per > 0.0 && (acc > per || acc < -per)) acc -= per * rint(acc / per);
  out[i] = (float)acc;
}

}  // namespace

namespace qmle {

int ensure_device_plan(qmle_plan *p) {
  if (p->dev.blob) {
    // the plan's device image lives on the device of its first run: refuse another one rather
    // than hand kernels a pointer they cannot read
    return p->dev.device == current_device() ? QMLE_OK : QMLE_ERR_UNSUPPORTED;
  }
  p->dev.device = current_device();
  const size_t b_ops = align_up(p->dev_ops.size() * sizeof(LoweredOp) + 16, 256);
  const size_t b_build = align_up(p->build_ops.size() * sizeof(BuildOp) + 16, 256);
  const size_t b_groups = align_up(p->groups.size() * sizeof(BuildGroup) + 16, 256);
  const size_t b_consts = align_up(p->consts.size() * sizeof(float) + 16, 256);
  const size_t b_opg = align_up(p->op_groups.size() * sizeof(OpGroup) + 16, 256);
  const size_t b_ops2 = align_up(p->ops2.size() * sizeof(LoweredOp) + 16, 256);
  const size_t b_grp2 = align_up(p->groups2.size() * sizeof(Group2) + 16, 256);
  const size_t b_tbl2 = align_up(p->tbl2.size() * sizeof(uint32_t) + 16, 256);
  const size_t total = b_ops + b_build + b_groups + b_consts + b_opg + b_ops2 + b_grp2 + b_tbl2;
  char *blob = nullptr;
  HIPCHK(hipMalloc((void **)&blob, total));
  p->dev.blob = blob;
  p->dev.blob_bytes = total;
  p->dev.d_ops = (LoweredOp *)blob;
  p->dev.d_build = (BuildOp *)(blob + b_ops);
  p->dev.d_groups = (BuildGroup *)(blob + b_ops + b_build);
  p->dev.d_consts = (float *)(blob + b_ops + b_build + b_groups);
  p->dev.d_op_groups = (OpGroup *)(blob + b_ops + b_build + b_groups + b_consts);
  char *fast = blob + b_ops + b_build + b_groups + b_consts + b_opg;
  p->dev.d_ops2 = (LoweredOp *)fast;
  p->dev.d_groups2 = (Group2 *)(fast + b_ops2);
  p->dev.d_tbl2 = (uint32_t *)(fast + b_ops2 + b_grp2);
  if (!p->ops2.empty())
    HIPCHK(hipMemcpy(p->dev.d_ops2, p->ops2.data(), p->ops2.size() * sizeof(LoweredOp),
                     hipMemcpyHostToDevice));
  if (!p->groups2.empty())
    HIPCHK(hipMemcpy(p->dev.d_groups2, p->groups2.data(), p->groups2.size() * sizeof(Group2),
                     hipMemcpyHostToDevice));
  if (!p->tbl2.empty())
    HIPCHK(hipMemcpy(p->dev.d_tbl2, p->tbl2.data(), p->tbl2.size() * sizeof(uint32_t),
                     hipMemcpyHostToDevice));
  if (!p->op_groups.empty())
    HIPCHK(hipMemcpy(p->dev.d_op_groups, p->op_groups.data(),
                     p->op_groups.size() * sizeof(OpGroup), hipMemcpyHostToDevice));
  if (!p->dev_ops.empty())
    HIPCHK(hipMemcpy(p->dev.d_ops, p->dev_ops.data(), p->dev_ops.size() * sizeof(LoweredOp),
                     hipMemcpyHostToDevice));
  if (!p->build_ops.empty())
    HIPCHK(hipMemcpy(p->dev.d_build, p->build_ops.data(),
                     p->build_ops.size() * sizeof(BuildOp), hipMemcpyHostToDevice));
  if (!p->groups.empty())
    HIPCHK(hipMemcpy(p->dev.d_groups, p->groups.data(), p->groups.size() * sizeof(BuildGroup),
                     hipMemcpyHostToDevice));
  if (!p->consts.empty())
    HIPCHK(hipMemcpy(p->dev.d_consts, p->consts.data(), p->consts.size() * sizeof(float),
                     hipMemcpyHostToDevice));
  return QMLE_OK;
}

// A run that starts from |0..0> keeps track of the amplitudes that are still exactly zero
// (Stage::zero_in).
bool plan_sparse(const qmle_plan *p) { return !(p->flags & QMLE_PLAN_NO_SPARSE); }

// qmle_run_batch_map hands its angle map to the matrix builder of the batch it is about to run (this
// thread's next launch_build_matrices of >= 64 samples): the angles are then formed inside the builder and
// the table is never written
static thread_local const AngleMapSrc *tls_angle_map = nullptr;
// whether this thread's next builder launch for `batch` samples takes its angles from the map (LastRun::matrices_from_map)
static bool builds_from_map(int batch) { return tls_angle_map && batch >= 64; }

// "this run's last stage ends in |amplitude|^2 only" (qmle_host.h), as the float offset its measured-mode records start at
uint32_t measured_records_from(const qmle_plan *p, int meas_type) {
  if (meas_type != QMLE_MEAS_EXPVAL_Z || p->stages.empty()) return 0xffffffffu;
  const Stage &st = p->stages.back();
  if (st.kind != ST_TILE || !st.fast_ok) return 0xffffffffu;
  uint32_t from = 0xffffffffu;
  for (int g = st.fast_begin; g < st.fast_end; ++g)
    if ((p->groups2[g].sync & kGroupProduct) && (p->groups2[g].sync & kGroupClosingFree) && p->groups2[g].prod_off < from)
      from = p->groups2[g].prod_off;
  // (records are appended stage by stage: the last stage's are the last of the row)
  return from;
}

// per-sample gate matrices for the whole batch: d_mats[b][mat_floats] from d_angles[b][n_slots]
int launch_build_matrices(const qmle_plan *p, const float *d_angles, float *d_mats, int batch, hipStream_t stream,
                          bool forward_only, uint32_t measured_from) {
  const int ng = forward_only ? p->n_groups_needed : (int)p->groups.size();
  if (ng <= 0) return QMLE_OK;
  // the product-form records of the fast groups: the last needed items, in a kernel of their own (the common
  // builder passes over them)
  const int npg = p->n_product_groups, pg0 = p->n_groups_needed - npg;
  const int ngc = forward_only ? pg0 : ng;  // items the common builder has work in
  if (builds_from_map(batch)) {
    const uint64_t per = ((uint64_t)batch + 63) / 64;
    if (ngc > 0)
      hipLaunchKernelGGL(k_build_matrices_map, dim3(grid_for((uint64_t)ngc * per * 64, 64)), dim3(64), 0, stream, p->dev.d_build,
                         p->dev.d_groups, ngc, *tls_angle_map, p->n_slots, p->dev.d_consts, d_mats, p->mat_floats, batch);
    if (npg > 0)
      hipLaunchKernelGGL(k_build_matrices_product_map, dim3(grid_for((uint64_t)npg * per * 64, 64)), dim3(64), 0, stream, p->dev.d_build,
                         p->dev.d_groups + pg0, npg, *tls_angle_map, p->n_slots, p->dev.d_consts, d_mats, p->mat_floats, batch, measured_from);
    HIPCHK(hipGetLastError());
    return QMLE_OK;
  }
  if (npg > 0) {
    const uint64_t pitems = batch >= 64 ? (uint64_t)npg * (((uint64_t)batch + 63) / 64) * 64 : (uint64_t)batch * (uint64_t)npg;
    if (batch >= 64)
      hipLaunchKernelGGL(k_build_matrices_product<true>, dim3(grid_for(pitems, 64)), dim3(64), 0, stream, p->dev.d_build,
                         p->dev.d_groups + pg0, npg, d_angles, p->n_slots, p->dev.d_consts, d_mats, p->mat_floats, batch, measured_from);
    else
      hipLaunchKernelGGL(k_build_matrices_product<false>, dim3(grid_for(pitems, 64)), dim3(64), 0, stream, p->dev.d_build,
                         p->dev.d_groups + pg0, npg, d_angles, p->n_slots, p->dev.d_consts, d_mats, p->mat_floats, batch, measured_from);
    HIPCHK(hipGetLastError());
    if (ngc <= 0) return QMLE_OK;
  }
  // one work item per (sample, group); from 64 samples on, whole waves per group (build_matrices_body)
  const uint64_t items = batch >= 64 ? (uint64_t)ngc * (((uint64_t)batch + 63) / 64) * 64 : (uint64_t)batch * (uint64_t)ngc;
  if (batch >= 64)
    hipLaunchKernelGGL(k_build_matrices<true>, dim3(grid_for(items, 64)), dim3(64), 0, stream, p->dev.d_build,
                       p->dev.d_groups, ngc, d_angles, p->n_slots, p->dev.d_consts, d_mats, p->mat_floats, batch);
  else
    hipLaunchKernelGGL(k_build_matrices<false>, dim3(grid_for(items, 64)), dim3(64), 0, stream, p->dev.d_build,
                       p->dev.d_groups, ngc, d_angles, p->n_slots, p->dev.d_consts, d_mats, p->mat_floats, batch);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

}  // namespace qmle

// ===========================================================================
// C ABI
// ===========================================================================
// (every qmle_* function below is declared extern "C" by include/qmle_sv.h; the definitions inherit it)

int qmle_sv_version(void) { return QMLE_SV_VERSION; }

const char *qmle_status_string(int status) {
  switch (status) {
    case QMLE_OK: return "ok";
    case QMLE_ERR_INVALID_ARG: return "invalid argument";
    case QMLE_ERR_WIRE_COUNT: return "wrong number of wires for gate";
    case QMLE_ERR_DUPLICATE_WIRES: return "duplicate wires";
    case QMLE_ERR_WIRE_RANGE: return "wire index out of range";
    case QMLE_ERR_UNKNOWN_OP: return "unknown opcode";
    case QMLE_ERR_MEAS_TYPE: return "unknown measurement type";
    case QMLE_ERR_WORKSPACE: return "workspace too small";
    case QMLE_ERR_HIP: return "HIP runtime error";
    case QMLE_ERR_NO_DEVICE: return "no HIP device";
    case QMLE_ERR_UNSUPPORTED: return "unsupported configuration";
    case QMLE_ERR_SLOT_RANGE: return "angle slot out of range";
    case QMLE_ERR_INTERNAL: return "internal invariant violated (kernel LDS layout)";
    default: return "unknown status";
  }
}

int qmle_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

// a new plan, not yet compiled, for `ops` on `base`'s register: its slots and the constants its caller handed in
// (without the permuted copies a compile appends).  NULL: out of memory.
static qmle_plan *new_plan_like(const qmle_plan *base, const std::vector<qmle_op> &ops, unsigned flags) {
  qmle_plan *c = new (std::nothrow) qmle_plan();
  if (!c) return nullptr;
  c->n = base->n;
  c->n_slots = base->n_slots;
  c->flags = flags;
  c->ops = ops;
  c->consts.assign(base->consts.begin(), base->consts.begin() + base->n_user_consts);
  c->n_user_consts = base->n_user_consts;
  return c;
}

int qmle_plan_create(const qmle_op *ops, int n_ops, int n_qubits, int n_slots,
                     const float *consts, int n_consts, unsigned flags, qmle_plan **out) {
  if (!out || n_ops < 0 || n_slots < 0 || n_consts < 0 || (n_ops > 0 && !ops))
    return QMLE_ERR_INVALID_ARG;
  *out = nullptr;
  if (flags & 16u) return QMLE_ERR_INVALID_ARG;  // reserved (include/qmle_sv.h)
  qmle_plan *p = new (std::nothrow) qmle_plan();
  if (!p) return QMLE_ERR_INVALID_ARG;
  flags &= ~QMLE_PLAN_INTERNAL_ZERO_RUN;  // internal: set below on the plans only qmle_run_batch executes
  p->n = n_qubits;
  p->n_slots = n_slots;
  p->flags = flags;
  p->ops.assign(ops, ops + n_ops);
  if (n_consts > 0) p->consts.assign(consts, consts + n_consts);
  p->n_user_consts = (size_t)(n_consts > 0 ? n_consts : 0);
  const int rc = compile_plan(p);
  if (rc != QMLE_OK) {
    delete p;
    return rc;
  }
  // The same tape scheduled for runs from |0..0> only (wider first tile): what qmle_run_batch
  // executes in place of `p` when the pass-cost model prefers it.  qmle_apply_inplace and the
  // adjoint sweep apply stages to LIVE states and keep `p`'s own schedule.
  if (!p->whole_state_lds && !(flags & QMLE_PLAN_NO_FUSION) &&
      !((flags >> 8) & 0xffffu) && p->stages.size() >= 2 && p->stages[0].kind == ST_TILE) {
    qmle_plan *v = new_plan_like(p, p->ops, flags | QMLE_PLAN_INTERNAL_ZERO_RUN);
    if (v) {
      const bool forced = std::getenv("QMLE_FORCE_CAND") != nullptr;  // (tuning: always run the forced schedule)
      if (compile_plan(v) == QMLE_OK && v->mat_floats_old == p->mat_floats_old && (forced || v->model_cost < p->model_cost - 0.5))
        p->zero_variant = v;
      else
        delete v;
    }
  }
  // <Z> measurements run a second plan without the trailing gates that only relabel basis
  // states or add phases (they are folded into the observables at run time)
  if (!(flags & (QMLE_PLAN_NO_ABSORB | QMLE_PLAN_NO_FUSION))) {
    std::vector<qmle_op> kept;
    split_expval_tail(p->ops, p->n, kept, p->absorbed);
    if (!p->absorbed.empty()) {
      // (a child only ever runs from |0..0>)
      qmle_plan *c = new_plan_like(p, kept, flags | QMLE_PLAN_NO_ABSORB | QMLE_PLAN_INTERNAL_ZERO_RUN);
      if (c) {
        for (const qmle_op &o : p->absorbed) p->absorbed_algo_bytes += algo_bytes(o, p->n);
        c->extra_algo_last_stage = p->absorbed_algo_bytes;
        if (compile_plan(c) == QMLE_OK) p->expval_child = c;
        else delete c;
        // Folding is not free any more (round 2): a folded CX tail turns <Z_w> into parities,
        // which the last tile pass measures with the general-mask epilogue (per tile: full
        // Walsh-Hadamard transform across the lanes) or, one-group passes on live input, with
        // k_reg_measure -- while the fast tile path applies X / CX for nothing (LDS layout) and
        // then takes the single-bit epilogue, whose sums stay in registers across a workgroup's
        // tiles.  Measured (MI355X, HE circuits, us per state, folded vs applied): n = 24: 2
        // layers 61.9 vs 45.5, 4 layers 115.8 vs 135.0; n = 22, 3 layers 25.4 vs 20.8; n = 20, 4
        // layers 8.9 vs 11.2.  The pass-cost model plus 17 (general-mask epilogue) resp. 12
        // (k_reg_measure on live input), in its units of 36 per read+write pass, picks the faster
        // plan in all of them; plans whose folded form ends in a known-zero special kernel keep it.
        if (p->expval_child && !c->stages.empty() && !c->whole_state_lds) {
          bool parity = false;
          for (int w = 0; w < p->n; ++w) {
            const uint32_t m = pull_back_z(p->absorbed, w);
            if (m & (m - 1u)) parity = true;
          }
          const size_t last = c->stages.size() - 1;
          const Stage &ls = c->stages[last];
          const int kind = expval_kernel_of(c, last, plan_sparse(c));
          double penalty = 0.0;
          if (ls.kind == ST_TILE && parity) {
            if (kind == 0) penalty = 17.0;
            else if (kind == 1 && (!plan_sparse(c) || ls.zero_in == 0)) penalty = 12.0;
          }
          const double applied_cost = p->zero_variant ? p->zero_variant->model_cost : p->model_cost;
          if (penalty > 0.0 && c->model_cost + penalty > applied_cost) {
            delete c;
            p->expval_child = nullptr;
          }
        }
      }
    }
    if (!p->expval_child) p->absorbed.clear();
  }
  *out = p;
  return QMLE_OK;
}
// the child that runs when trailing gates were folded into the Z observables (NULL: nothing was folded)
qmle_plan *qmle_plan_expval_child(qmle_plan *plan) { return plan ? plan->expval_child : nullptr; }
// the plan qmle_run_batch really executes for `meas_type`: the folded child for QMLE_MEAS_EXPVAL_Z when
// there is one, and of that (or of the plan) the schedule compiled for runs from |0..0> when the
// pass-cost model preferred it.  Never NULL for a valid plan; describe / profile THIS handle.
qmle_plan *qmle_plan_executed(qmle_plan *plan, int meas_type) {
  if (!plan) return nullptr;
  qmle_plan *p = (meas_type == QMLE_MEAS_EXPVAL_Z && plan->expval_child) ? plan->expval_child : plan;
  return p->zero_variant ? p->zero_variant : p;
}

int qmle_plan_destroy(qmle_plan *plan) {
  if (!plan) return QMLE_OK;
  if (plan->expval_child) (void)qmle_plan_destroy(plan->expval_child);
  if (plan->zero_variant) (void)qmle_plan_destroy(plan->zero_variant);
  if (plan->adj_blob) (void)hipFree(plan->adj_blob);
  if (plan->adjf_blob) (void)hipFree(plan->adjf_blob);
  if (plan->f64_blob) (void)hipFree(plan->f64_blob);
  if (plan->dev.blob) (void)hipFree(plan->dev.blob);
  delete plan;
  return QMLE_OK;
}

// the matrix builder's chain walk (unit_chain_step, qmle_matrices.h) on the host, for given 2x2 matrices
int qmle_unit_form_chain(const double *u, const int *diag, int n, double *records, double *pivots, double *carrier) {
  if (!u || n < 1 || !carrier || (n > 1 && (!records || !pivots))) return QMLE_ERR_INVALID_ARG;
  cd P = {1.0, 0.0};
  for (int i = 0; i < n; ++i) {
    const double *m = u + 8 * (size_t)i;
    const M2 U = {{m[0], m[1]}, {m[2], m[3]}, {m[4], m[5]}, {m[6], m[7]}};
    if (i + 1 == n) {
      (void)unit_chain_step(U, CM_CARRIER, P, carrier);
    } else {
      const cd piv = unit_chain_step(U, diag && diag[i] ? CM_UNIT_DIAG : CM_UNIT_DENSE, P, records + 8 * (size_t)i);
      pivots[2 * i] = piv.re;
      pivots[2 * i + 1] = piv.im;
    }
  }
  return QMLE_OK;
}

// the matrix builder's product form of a group (product_form_group, qmle_matrices.h) on the host: n <= 4 matrices
// (8 doubles each, row-major re / im) on the distinct in-thread bits `bits`; record: kProductRecFloats doubles
static int group_product_form(const double *u, const int *bits, int n, double *record, int *forms, bool measured) {
  if (!u || !bits || !record || n < 1 || n > 4) return QMLE_ERR_INVALID_ARG;
  M2 m[4];
  unsigned seen = 0;
  for (int i = 0; i < n; ++i) {
    if (bits[i] < 0 || bits[i] > 3 || (seen & (1u << bits[i]))) return QMLE_ERR_INVALID_ARG;
    seen |= 1u << bits[i];
    const double *x = u + 8 * (size_t)i;
    m[i] = {{x[0], x[1]}, {x[2], x[3]}, {x[4], x[5]}, {x[6], x[7]}};
  }
  product_form_group(m, bits, n, record, forms, measured);
  return QMLE_OK;
}
int qmle_group_product_form(const double *u, const int *bits, int n, double *record, int *forms) {
  return group_product_form(u, bits, n, record, forms, /*measured=*/false);
}
// ... in measured mode: the record of a run in which only basis permutations and |amplitude|^2 follow the group
int qmle_group_product_form_measured(const double *u, const int *bits, int n, double *record, int *forms) {
  return group_product_form(u, bits, n, record, forms, /*measured=*/true);
}

int qmle_plan_describe(const qmle_plan *plan, char *buf, size_t cap) {
  if (!plan) return QMLE_ERR_INVALID_ARG;
  const std::string s = describe_plan(plan);
  if (buf && cap > 0) {
    const size_t nc = s.size() < cap - 1 ? s.size() : cap - 1;
    std::memcpy(buf, s.data(), nc);
    buf[nc] = 0;
  }
  return (int)s.size();
}

int qmle_plan_stats(const qmle_plan *plan, int64_t stats[8]) {
  if (!plan || !stats) return QMLE_ERR_INVALID_ARG;
  int direct = 0;
  for (const Stage &s : plan->stages) direct += s.kind == ST_DIRECT;
  stats[0] = (int64_t)plan->ops.size();
  stats[1] = (int64_t)plan->stages.size();
  stats[2] = plan->whole_state_lds ? 1 : 0;
  stats[3] = plan->tile_T;
  stats[4] = plan->mat_floats;
  stats[5] = direct;
  stats[6] = (int64_t)plan->lowered.size();
  stats[7] = (int64_t)plan->algo_bytes_per_state;
  return QMLE_OK;
}

static size_t ws_matrix_bytes(const qmle_plan *p, int batch) {
  return align_up((size_t)batch * (p->mat_floats ? p->mat_floats : 1) * sizeof(float), 256);
}
// per-sample gate matrices, then the product stages' group columns (k_fold_columns)
size_t qmle::ws_mats_bytes(const qmle_plan *p, int batch) {
  return ws_matrix_bytes(p, batch) +
         align_up((size_t)batch * (size_t)p->fold_groups * 16 * sizeof(float2), 256) +
         align_up((size_t)batch * 32 * sizeof(float), 256);  // k_mono_coef
}

static int default_states_in_flight(const qmle_plan *p, int batch) {
  // states per launch: the tile passes are LDS/VALU-bound, so big launches (fewer tails)
  // beat Infinity-Cache residency -- measured 3.4k -> 4.1k statevectors/s at n = 24 going
  // from 1 to 32 states in flight, +1 % more at 128 (profiles/r01_in_flight_sweep.txt); runs
  // that skip known zeros are launch-bound at 32 (11.5 M -> 14.3 M -> 15.2 M gate-applies/s at
  // 32 / 128 / 512 states, K2).  32 GiB of state buffers = 256 states at n = 24.
  // Round 2: a plan whose every pass streams the whole state (no known zeros left to skip) is
  // not launch-bound, and its passes run faster on a 4 GiB than on a 32 GiB working set -- K2
  // all-live at n = 24: 111.0 / 111.6 / 108.3 / 107.2 / 107.7 ms per 1024 states for 32 / 16 /
  // 8 / 4 / 2 GiB per launch (the read+write pass: 56.6 vs 51.6 us per state at 256 vs 64
  // states); the known-zero plans keep 32 GiB (3.0 vs 4.9 ms per step at 4 GiB).
  const size_t sb = (size_t)8 << p->n;
  bool whole_state_every_pass = p->stages.size() >= 2;
  if (plan_sparse(p))
    for (size_t si = 1; si < p->stages.size(); ++si)
      if (p->stages[si].zero_in != 0) whole_state_every_pass = false;
  const size_t budget_mib = whole_state_every_pass ? 4096 : 32768;
  size_t s = (budget_mib << 20) / sb;
  if (s < 1) s = 1;
  if (s > (size_t)batch) s = (size_t)batch;
  return (int)s;
}

static size_t expval_partial_rows(const qmle_plan *p) {
  size_t rows = (size_t)expval_blocks(p->n);
  if ((size_t)overlap_blocks(p->n) > rows) rows = (size_t)overlap_blocks(p->n);
  if (!p->stages.empty() && p->stages.back().kind == ST_TILE && !p->whole_state_lds) {
    const size_t tiles = (size_t)1 << (p->n - p->stages.back().T);
    if (tiles > rows) rows = tiles;
  }
  return rows;
}

// Meyer-Wallach measurement: can the plan's last pass report its tile's sums (tile_mw_row)?
// Policy (measured on MI355X): when the last pass holds the WHOLE state (n <= 14) the sums cost
// one epilogue and no statevector is ever stored -- always taken.  For tiled states the round-4 epilogue (208
// packed fmas + a 41-value wave reduction per work item and tile) cost the pass what the saved read was worth
// (n = 28: 0.99 ms after the circuit either way) and stayed opt-in; since round 5 the producing pass leaves positions
// 0..3 to the first later read (lean epilogue) and streams its stores, so that the later reads do not run into its
// write-back: 0.79 ms after the circuit against 0.92-1.0 for the stand-alone reads -- taken by default
// (QMLE_MW_FUSE_TILED=0: the stand-alone reads; read per call: A/B, tests).
static bool plan_mw_fusable(const qmle_plan *p) {
  if (p->stages.empty()) return false;
  const Stage &last = p->stages.back();
  // (round 5: tiled states fuse by default -- lean epilogue + streaming stores, n = 28: 0.81 ms after the circuit
  // against 1.0 ms for the three stand-alone reads)
  const char *ft = std::getenv("QMLE_MW_FUSE_TILED");
  if (last.T < p->n && ft && atoi(ft) == 0) return false;
  return mw_fusable(p->n, last);
}
// rows + purities of `batch` states (conservative per state: the rows per state shrink with the batch)
static size_t mw_ws_bytes(const qmle_plan *p, int batch) {
  // (enough for either route: QMLE_MW_FUSE_TILED is read per call, a workspace sized before it was flipped stays valid)
  size_t one = mw_resident_ws_bytes(p->n, 1);
  if (!p->stages.empty() && mw_fusable(p->n, p->stages.back()))
    one = std::max(one, mw_fused_ws_bytes(p->n, 1, p->stages.back()));
  return align_up(one, 256) * (size_t)batch;
}

// Round 5: consecutive chunks of a batch are independent (own states, own partial sums), and their passes want
// different things from the GPU -- the zero fill HBM writes, the one-tile-per-state kernel 32 workgroups, a measuring
// pass the vector unit.  Two processes sharing the card ran the all-live K2 step 18 % faster than one (1.93 against 1.63 M
// gate-applies/s); the same overlap inside one call: chunks alternate between two internal streams that fork from the
// caller's stream and join it again.  QMLE_NO_CHUNK_OVERLAP=1: the one-stream loop (read per call).
static bool chunk_overlap_on() { return std::getenv("QMLE_NO_CHUNK_OVERLAP") == nullptr; }
constexpr int kPipeStages = 32;
struct SideStreams {
  hipStream_t s[2] = {nullptr, nullptr};
  hipEvent_t fork = nullptr, join[2] = {nullptr, nullptr};
  // software pipeline: stage k of chunk i + 1 starts when stage k of chunk i is done -- two chunks in lockstep
  // (fill next to fill, measuring pass next to measuring pass) share the card evenly and gain nothing; one stage
  // apart, the HBM-bound pass of one chunk runs beside the vector-bound pass of the other
  hipEvent_t stage_done[2][kPipeStages] = {};
  // measuring passes alone on s[0] (ChunkPipeline, the `alone` form): per slot, the chunk's first pass is queued on
  // s[1] / its measuring pass is queued on s[0]
  hipEvent_t first_done[2] = {nullptr, nullptr}, walk_done[2] = {nullptr, nullptr};
  bool ok = false;
};
static SideStreams *side_streams() {
  static SideStreams per_dev[kMaxDevices];
  static std::mutex mu;
  const int dev = current_device();
  if (dev < 0 || dev >= kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  SideStreams &x = per_dev[dev];
  if (!x.ok) {
    bool good = hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess;
    for (int k = 0; k < 2 && good; ++k) {
      good = hipStreamCreateWithFlags(&x.s[k], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&x.join[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&x.first_done[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&x.walk_done[k], hipEventDisableTiming) == hipSuccess;
      for (int e = 0; e < kPipeStages && good; ++e)
        good = hipEventCreateWithFlags(&x.stage_done[k][e], hipEventDisableTiming) == hipSuccess;
    }
    if (!good) { (void)hipGetLastError(); return nullptr; }
    x.ok = true;
  }
  return &x;
}

// Workspace of qmle_run_batch, from the first 256-byte boundary of the caller's pointer on:
//   [matrix rows: batch * mat_floats] [columns of the product stages' groups] [k_mono_coef table]
//   slot 0: [states of a chunk: in_flight * 2^n] [partial sums / Meyer-Wallach rows of the chunk]
//   slot 1: the same again, when the chunks alternate between the two internal streams (ChunkPipeline)
// One function fills it, for the size query and for the run.
struct BatchLayout {
  size_t cols = 0, coef = 0;  // fold columns (k_fold_columns), k_mono_coef table; the matrix rows sit at 0
  bool in_lds = false;        // one launch simulates and measures: no state is stored (run_batch_lds)
  int in_flight = 0;          // states per chunk
  int slots = 1;
  size_t states[2] = {}, partial[2] = {};  // per slot (states: not used when the chunks are rows of d_out)
  size_t partial_bytes = 0;                // of one slot
  size_t total = 0;                        // with the slack for aligning the caller's pointer
};
// handed == NULL: the layout for chunks of `asked` states (<= 0: the default), i.e. the size query.  Otherwise the
// layout for a workspace of *handed bytes (a caller may hand in less than the query said): fewer states per chunk,
// then one slot instead of two; false: not even one state fits.  side: whether the side streams exist, when the
// caller knows (qmle_chunk_loop_form, which makes no HIP call); -1: ask for them.
static bool batch_layout(const qmle_plan *plan, int batch, int meas_type, int asked, const size_t *handed,
                         BatchLayout &L, int side = -1) {
  L.cols = ws_matrix_bytes(plan, batch);
  L.coef = L.cols + align_up((size_t)batch * (size_t)plan->fold_groups * 16 * sizeof(float2), 256);
  const size_t base = ws_mats_bytes(plan, batch);
  if (handed && *handed < base) return false;
  const size_t room = handed ? *handed - base : ~(size_t)0;
  L.total = base + 512;
  L.states[0] = L.partial[0] = base;
  // a chunk's partial sums: rows of the <Z> epilogues, or Meyer-Wallach rows + purities
  const size_t partial_one =
      meas_type == QMLE_MEAS_EXPVAL_Z ? align_up(expval_partial_rows(plan) * (QMLE_MAX_QUBITS + 1) * sizeof(float), 256)
      : meas_type == QMLE_MEAS_MEYER_WALLACH ? mw_ws_bytes(plan, 1) : 0;
  if (plan->whole_state_lds &&
      (meas_type == QMLE_MEAS_STATE || meas_type == QMLE_MEAS_PROBS || meas_type == QMLE_MEAS_EXPVAL_Z ||
       (meas_type == QMLE_MEAS_MEYER_WALLACH && plan_mw_fusable(plan)))) {
    // the state never leaves the LDS; the Meyer-Wallach sums come out of the tile as one block of rows
    L.in_lds = true;
    L.in_flight = handed ? std::min(batch, kMaxGridY) : batch;
    L.partial_bytes = (size_t)L.in_flight * partial_one;
    if (meas_type != QMLE_MEAS_MEYER_WALLACH) return true;
    L.total += L.partial_bytes;
    return room >= L.partial_bytes;
  }
  // QMLE_MEAS_STATE: every chunk is its own rows of d_out (sample-major: stay cache-resident)
  const size_t state_one = align_up((size_t)8 << plan->n, 256);
  const size_t per = meas_type == QMLE_MEAS_STATE ? 0 : state_one + partial_one;
  const size_t dflt = (size_t)default_states_in_flight(plan, batch);
  size_t s = handed || asked <= 0 ? dflt : (size_t)asked;
  if (handed && per) s = std::min(s, room / per);
  if (s < 1) return false;
  s = std::min(s, (size_t)batch);
  if (handed) s = std::min(s, (size_t)kMaxGridY);
  // Two slots -- chunks alternate between two internal streams, each with its own state / partial buffers: the
  // batch has several chunks, the overlap switch is on, the plan is not one streaming pass per gate
  // (QMLE_PLAN_NO_FUSION is HBM-bound in every pass: two of them at once share the bandwidth and lose 2-3 % to the
  // mix), the side streams exist, and there is room for two.  A workspace sized by the query holds two slots of the
  // chunk it was asked for; one that holds less is split in two.
  // The size query cannot ask for the streams, and it does not look at QMLE_PLAN_NO_FUSION either: for those plans
  // it reserves a second slot that the run leaves unused.  Sizes stay as they are in this change.
  bool two = s < (size_t)batch && chunk_overlap_on();
  if (two && handed) {
    size_t half = s;
    if (per) half = std::min(std::min(room / per / 2, dflt), (size_t)kMaxGridY);
    two = !(plan->flags & QMLE_PLAN_NO_FUSION) && half >= 1 && (side < 0 ? side_streams() != nullptr : side != 0);
    if (two) s = half;
  }
  L.in_flight = (int)s;
  L.slots = two ? 2 : 1;
  L.partial_bytes = s * partial_one;
  for (int k = 0; k < L.slots; ++k) {
    L.states[k] = base + (size_t)k * s * per;
    L.partial[k] = L.states[k] + (per ? s * state_one : 0);
  }
  L.total += (size_t)L.slots * s * per;
  return true;
}

size_t qmle::workspace_bytes_one(const qmle_plan *plan, int batch, int meas_type,
                                 int states_in_flight) {
  BatchLayout L;
  batch_layout(plan, batch, meas_type, states_in_flight, nullptr, L);
  return L.total;
}

size_t qmle_workspace_bytes(const qmle_plan *plan, int batch, int meas_type, int n_obs,
                            int states_in_flight) {
  (void)n_obs;
  if (!plan || batch < 1) return 0;
  size_t total = workspace_bytes_one(plan, batch, meas_type, states_in_flight);
  if (plan->zero_variant) {
    const size_t c = workspace_bytes_one(plan->zero_variant, batch, meas_type, states_in_flight);
    if (c > total) total = c;
  }
  if (meas_type == QMLE_MEAS_EXPVAL_Z && plan->expval_child) {
    const size_t c = workspace_bytes_one(plan->expval_child, batch, meas_type, states_in_flight);
    if (c > total) total = c;
  }
  return total;
}



// <Z..Z> on wire masks (bit w = wire w), pulled back through the folded tail -> position masks
static int build_obs_masks(qmle_plan *plan, qmle_plan **exec, const uint32_t *wire_masks, int n_obs,
                           uint32_t *masks) {
  const int n = plan->n;
  *exec = plan->expval_child ? plan->expval_child : plan;
  for (int k = 0; k < n_obs; ++k) {
    const uint32_t in = wire_masks[k];
    if (!valid_wire_mask(in, n)) return QMLE_ERR_WIRE_RANGE;
    uint32_t wm = 0;  // a product of Z's pulls back to the XOR of the factors' pull-backs
    for (int w = 0; w < n; ++w)
      if (in & (1u << w)) wm ^= *exec == plan ? 1u << w : pull_back_z(plan->absorbed, w);
    masks[k] = wires_to_pos(wm, n);  // (never 0: the pull-back is an invertible linear map)
  }
  return QMLE_OK;
}

static int run_batch_checked(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                             const int32_t *obs_wires, int n_obs, void *d_out, void *d_workspace,
                             size_t workspace_bytes, qmle_stream stream_, uint64_t *ws_token);

int qmle_run_batch(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                   const int32_t *obs_wires, int n_obs, void *d_out, void *d_workspace,
                   size_t workspace_bytes, qmle_stream stream_) {
  return qmle_run_batch_w(plan, d_angles, batch, meas_type, obs_wires, n_obs, d_out, d_workspace, workspace_bytes,
                          stream_, nullptr);
}

// every error return voids the caller's token (run_batch_masks does the same for its own)
static int void_token(uint64_t *ws_token, int rc) {
  if (ws_token) *ws_token = 0;
  return rc;
}

int qmle_run_batch_w(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                     const int32_t *obs_wires, int n_obs, void *d_out, void *d_workspace,
                     size_t workspace_bytes, qmle_stream stream_, uint64_t *ws_token) {
  const int rc = run_batch_checked(plan, d_angles, batch, meas_type, obs_wires, n_obs, d_out, d_workspace,
                                   workspace_bytes, stream_, ws_token);
  return rc == QMLE_OK ? rc : void_token(ws_token, rc);
}

static int run_batch_checked(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                             const int32_t *obs_wires, int n_obs, void *d_out, void *d_workspace,
                             size_t workspace_bytes, qmle_stream stream_, uint64_t *ws_token) {
  if (!plan || batch < 1 || !d_out || !d_workspace) return QMLE_ERR_INVALID_ARG;
  if (meas_type < QMLE_MEAS_STATE || meas_type > QMLE_MEAS_MEYER_WALLACH) return QMLE_ERR_MEAS_TYPE;
  if (plan->n_slots > 0 && !d_angles) return QMLE_ERR_INVALID_ARG;
  uint32_t masks[QMLE_MAX_QUBITS];
  qmle_plan *exec = plan;
  if (meas_type == QMLE_MEAS_EXPVAL_Z) {
    if (n_obs < 1 || n_obs > QMLE_MAX_QUBITS || !obs_wires) return QMLE_ERR_INVALID_ARG;
    uint32_t wm[QMLE_MAX_QUBITS];
    for (int k = 0; k < n_obs; ++k) {
      if (obs_wires[k] < 0 || obs_wires[k] >= plan->n) return QMLE_ERR_WIRE_RANGE;
      wm[k] = 1u << obs_wires[k];
    }
    const int rc = build_obs_masks(plan, &exec, wm, n_obs, masks);
    if (rc != QMLE_OK) return rc;
  }
  return run_batch_masks(exec, d_angles, batch, meas_type, masks, n_obs, d_out, d_workspace,
                         workspace_bytes, (hipStream_t)stream_, ws_token);
}

int qmle_run_batch_parity(qmle_plan *plan, const float *d_angles, int batch,
                          const uint32_t *wire_masks, int n_obs, float *d_out, void *d_workspace,
                          size_t workspace_bytes, qmle_stream stream_) {
  return qmle_run_batch_parity_w(plan, d_angles, batch, wire_masks, n_obs, d_out, d_workspace, workspace_bytes,
                                 stream_, nullptr);
}

int qmle_run_batch_parity_w(qmle_plan *plan, const float *d_angles, int batch,
                            const uint32_t *wire_masks, int n_obs, float *d_out, void *d_workspace,
                            size_t workspace_bytes, qmle_stream stream_, uint64_t *ws_token) {
  if (!plan || batch < 1 || !d_out || !d_workspace || !wire_masks || n_obs < 1 ||
      n_obs > QMLE_MAX_QUBITS)
    return void_token(ws_token, QMLE_ERR_INVALID_ARG);
  if (plan->n_slots > 0 && !d_angles) return void_token(ws_token, QMLE_ERR_INVALID_ARG);
  uint32_t masks[QMLE_MAX_QUBITS];
  qmle_plan *exec = plan;
  const int rc = build_obs_masks(plan, &exec, wire_masks, n_obs, masks);
  if (rc != QMLE_OK) return void_token(ws_token, rc);
  return run_batch_masks(exec, d_angles, batch, QMLE_MEAS_EXPVAL_Z, masks, n_obs, d_out,
                         d_workspace, workspace_bytes, (hipStream_t)stream_, ws_token);
}

// How a run reads its <Z> observables (bit-position parity masks).
struct ObsClass {
  bool single_bits = true;   // plain Z observables: the 33-sums epilogue serves them all
  bool semi_single = false;  // parities that meet the last tile in at most one position (below)
  ObsBits by_position;       // column of the 33-float row = the observable's position (+ row signs: semi_single)
  ObsBits by_index;          // column k = observable k (general-mask epilogue, k_reg_measure)
};
static ObsClass classify_observables(const qmle_plan *plan, const uint32_t *obs_masks, int n_obs) {
  ObsClass oc;
  const int n = plan->n;
  for (int k = 0; k < n_obs; ++k) {
    const uint32_t m = obs_masks[k];
    if (m == 0 || (m & (m - 1))) oc.single_bits = false;
    oc.by_position.bits[k] = (int8_t)(m ? __builtin_ctz(m) : 0);
    oc.by_index.bits[k] = (int8_t)k;
  }
  // Parities that touch the LAST tile in at most one position (the rest are outer positions =
  // bits of the tile index) also come out of the 33-sums epilogue: column of that position (or
  // of the total) summed over the tile rows with the sign of the outer part; the general-mask
  // epilogue costs 13 - 17 us per state at n = 24, this one 4 - 6.  (A CX tail that would make
  // every folded parity of an HE ring meet the last tile in one position does not exist: the
  // restrictions of those parities to T wires are T + 1 or T + 2 distinct ranges.)
  if (!oc.single_bits && !plan->stages.empty() && plan->stages.back().kind == ST_TILE && !plan->whole_state_lds) {
    const Stage &ls = plan->stages.back();
    uint32_t tile_mask = 0;
    for (int j = 0; j < ls.T; ++j) tile_mask |= 1u << ls.tile_bits[j];
    oc.semi_single = true;
    for (int k = 0; k < n_obs && oc.semi_single; ++k) {
      const uint32_t m = obs_masks[k], in = m & tile_mask;
      if (m == 0 || (in & (in - 1u))) { oc.semi_single = false; break; }
      oc.by_position.bits[k] = (int8_t)(in ? __builtin_ctz(in) : QMLE_MAX_QUBITS);  // column 32: the tile's total
      uint32_t rm = 0;
      for (int i = 0; i < n - ls.T; ++i)
        if ((m >> ls.outer_bits[i]) & 1u) rm |= 1u << i;
      oc.by_position.row_mask[k] = rm;
    }
  }
  return oc;
}

// LastRun: whether the last launch of tile stage `si` ran its product-form groups
static void note_product_form(qmle_plan *plan, size_t si, const TileRoute &route) {
  if (si < 64) plan->last_run.product_form_stages = (plan->last_run.product_form_stages & ~(1ull << si)) | ((uint64_t)route.product_form << si);
}
// ... of a batch run: whether its last stage ran records the builder wrote in measured mode (LastRun::measured_form)
static void note_product_form(qmle_plan *plan, size_t si, const TileRoute &route, int meas_type) {
  note_product_form(plan, si, route);
  if (si + 1 == plan->stages.size())
    plan->last_run.measured_form = route.product_form && measured_records_from(plan, meas_type) != 0xffffffffu;
}

// The whole state lives in the LDS of one workgroup: one launch per chunk simulates and measures, and the state
// is stored only when the state is what was asked for.  `rows`: the Meyer-Wallach rows of a chunk (L.partial_bytes).
static int run_batch_lds(qmle_plan *plan, const BatchLayout &L, const float *d_mats, const float *d_angles, int batch,
                         int meas_type, const uint32_t *obs_masks, int n_obs, void *d_out, void *rows,
                         hipStream_t stream) {
  const Stage &st = plan->stages[0];
  const int n = plan->n;
  const size_t D = (size_t)1 << n;
  for (int b0 = 0; b0 < batch; b0 += L.in_flight) {
    const int bc = std::min(batch - b0, L.in_flight);
    const float *mats = d_mats + (size_t)b0 * plan->mat_floats;
    const float *ang = d_angles ? d_angles + (size_t)b0 * plan->n_slots : nullptr;
    ProfScope prof_scope(plan, 0, stream);
    TileBuffers tb{nullptr, mats, ang};
    TileRequest rq;
    rq.batch = bc;
    rq.init_zero = true;
    if (meas_type == QMLE_MEAS_STATE) {
      tb.states = (float2 *)d_out + (size_t)b0 * D;
      rq.meas = TM_STORE;
    } else if (meas_type == QMLE_MEAS_PROBS) {
      tb.out = (float *)d_out + (size_t)b0 * D;
      rq.meas = TM_PROBS;
    } else if (meas_type == QMLE_MEAS_EXPVAL_Z) {
      tb.out = (float *)d_out + (size_t)b0 * n_obs;
      tb.obs_masks = obs_masks;
      rq.meas = TM_EXPVAL;
      rq.n_obs = n_obs;
    } else {  // circuit + Meyer-Wallach sums
      tb.out = rows;
      rq.meas = TM_MW_ONLY;
    }
    TileRoute route;
    int rc = launch_tile(plan, 0, tb, rq, stream, &route);
    note_product_form(plan, 0, route, meas_type);
    if (rc == QMLE_OK && meas_type == QMLE_MEAS_MEYER_WALLACH)
      rc = run_mw_fused(nullptr, n, bc, st, 0, rows, L.partial_bytes, (float *)d_out + (size_t)b0 * (n + 1), stream,
                        &plan->last_run.mw_finish);
    if (rc != QMLE_OK) return rc;
  }
  return QMLE_OK;
}

// The two-stream pipeline of a batch's chunks (round 5, above SideStreams): chunk i runs on internal stream i & 1
// with workspace slot i & 1.  The streams fork from the caller's stream -- what it has queued so far (the matrices,
// the angle table) comes first -- and join it again when the object goes, on the error returns too.  Without side
// streams (one slot, or a fork that failed) every chunk runs on the caller's stream in slot 0.
//
// Between the two streams, three loop forms (chunk_loop_form decides, form() is reported as chunk_loop_last_run):
//   staged  stage k of chunk i + 1 waits, by event, for stage k of chunk i: at most one launch of each stage in flight,
//           the chunks one stage apart.  Every run whose chunks are filled one by one.
//   free    no event between the streams: each stream runs its chunks back to back, and the tail of one chunk's
//           measuring pass -- the last walks draining, the launch of the next kernel -- is covered by the other
//           stream's pass.  For runs whose slots stay zeroed (slot_stays_zeroed: one fill per slot and call, so in
//           steady state the staged rule only put one measuring pass behind the other).  What orders such a run: a
//           slot is one buffer on one stream; the matrix rows, the plan's tables and the observables are read-only;
//           output rows, partial sums, fold columns and the k_mono_coef rows are per chunk or per slot.
//   alone   for the runs of the free form whose measuring pass is HBM-bound (a launch alone on the card takes 0.684 ms,
//           two sharing it 1.394 ms each): s[0] carries the measuring passes and nothing else, one after
//           the other; s[1] carries every chunk's first pass and epilogue.  Per slot k two events: first_done[k] lets the
//           measuring pass of a chunk start behind its first pass, walk_done[k] lets the chunk's epilogue start -- and
//           the first pass of the next chunk in that slot, which stores into the state buffer the pass reads.  The
//           partial sums of a slot are read by the epilogue of chunk i in front of the first pass of chunk i + 2 on
//           s[1], which the measuring pass that rewrites them waits for.  s[1] runs in order, so run_batch_chunks
//           queues the first pass of chunk i + 1 in front of the epilogue of chunk i: behind it, it would wait for
//           the measuring pass of chunk i and leave s[0] idle while it runs.  (Measured: a first pass is 32 workgroups
//           of 1024 work items and 128 KiB of LDS, and no CU has that much free while a measuring pass still has
//           workgroups to place, so it runs in the tail of the pass it was queued beside and ends 28 us behind it;
//           the next measuring pass starts 50 us after the last one ended.  A stream of the highest priority for
//           the first passes changes nothing.)
class ChunkPipeline {
 public:
  // the parts of a chunk, in the order every form but `alone` queues them: stage 0 (with its fill), the stages behind
  // it (of a run that takes the `alone` form: the measuring pass), the measurement behind the last stage
  enum Part { kFirst = 0, kMeasure, kEpilogue };
  // form: chunk_loop_form's (a fork that fails leaves the one-stream loop)
  ChunkPipeline(int form, hipStream_t caller_stream) : caller_(caller_stream), form_(form) {
    side_ = form != kChunkLoopOneStream ? side_streams() : nullptr;
    if (side_ && (hipEventRecord(side_->fork, caller_) != hipSuccess ||
                  hipStreamWaitEvent(side_->s[0], side_->fork, 0) != hipSuccess ||
                  hipStreamWaitEvent(side_->s[1], side_->fork, 0) != hipSuccess)) {
      (void)hipGetLastError();
      side_ = nullptr;
    }
    if (!side_) form_ = kChunkLoopOneStream;
  }
  ChunkPipeline(const ChunkPipeline &) = delete;
  ChunkPipeline &operator=(const ChunkPipeline &) = delete;
  ~ChunkPipeline() {
    if (!side_) return;
    for (int k = 0; k < 2; ++k)
      if (hipEventRecord(side_->join[k], side_->s[k]) == hipSuccess)
        (void)hipStreamWaitEvent(caller_, side_->join[k], 0);
  }
  int slot(int chunk) const { return side_ ? chunk & 1 : 0; }
  hipStream_t stream(int chunk, Part part) const {
    if (!side_) return caller_;
    return side_->s[form_ == kChunkLoopAlone ? (part == kMeasure ? 0 : 1) : chunk & 1];
  }
  // What a stage or a part waits for is queued here; the result marks it as queued itself when it goes out of scope
  // (any exit from the stage's iteration / the part's function).
  struct Queued {
    hipEvent_t ev;
    hipStream_t stream;
    ~Queued() { if (ev) (void)hipEventRecord(ev, stream); }
  };
  // Staged form: stage k of chunk i starts behind stage k of chunk i - 1 (the other stream).  Other forms: nothing to do.
  Queued begin_stage(int chunk, size_t k, hipStream_t stream) const {
    const bool piped = form_ == kChunkLoopStaged;
    if (piped && chunk > 0) (void)hipStreamWaitEvent(stream, side_->stage_done[(chunk - 1) & 1][k], 0);
    return Queued{piped ? side_->stage_done[chunk & 1][k] : nullptr, stream};
  }
  // `alone` form: the events of the chunk's slot (above).  Other forms: nothing to do.
  Queued begin_part(int chunk, Part part) const {
    const hipStream_t st = stream(chunk, part);
    if (form_ != kChunkLoopAlone) return Queued{nullptr, st};
    const int k = chunk & 1;
    if (part == kMeasure) {
      (void)hipStreamWaitEvent(st, side_->first_done[k], 0);
      return Queued{side_->walk_done[k], st};
    }
    // (the slot's first chunk: walk_done[k] has not been recorded in this run, and the fork orders it behind earlier ones)
    if (part == kEpilogue || chunk >= 2) (void)hipStreamWaitEvent(st, side_->walk_done[k], 0);
    return Queued{part == kFirst ? side_->first_done[k] : nullptr, st};
  }
  // how this run orders its chunks (LastRun::chunk_loop)
  int form() const { return form_; }

 private:
  SideStreams *side_;
  hipStream_t caller_;
  int form_;
};

// Does a workspace slot still hold what the filled first pass of a chunk left in it -- zeros everywhere outside tile 0
// of each state -- when the chunk is done?  Then the next chunk in that slot needs no fill (launch_tile).  True when
// no launch of the chunk loop behind stage 0 stores into the chunk's state buffer.  Admitted, each read to take the
// state as input only: the last tile pass of a two-stage plan with its <Z> epilogue -- launch_tile with
// TM_EXPVAL_PARTIAL / TM_EXPVAL_MASKS (k_tile2's measuring instantiations, k_tile + tile_epilogue: rows of partial
// sums to `out`) or routed to k_reg_measure* (k_reg_measure, k_reg_measure_mono: const loads, rows to `out`) -- and
// launch_expval_final behind it (reads the rows).
// Every other run fills every chunk: any TM_STORE / TM_STORE_MW pass or run_stage_inplace behind stage 0 (so every
// plan of three or more stages, and two-stage plans measured otherwise than by the fused <Z> epilogue), one-stage
// plans, probabilities, the Meyer-Wallach reads and launch_density (read-only or not: not admitted here), and
// QMLE_MEAS_STATE, whose chunks are rows of d_out and never share a buffer.
static bool slot_stays_zeroed(const qmle_plan *plan, bool fuse_expval) {
  // (fuse_expval: QMLE_MEAS_EXPVAL_Z, and the last stage is a tile stage that measures instead of storing)
  return plan->stages.size() == 2 && plan->stages[0].kind == ST_TILE && fuse_expval;
}
// <Z> straight out of the last tile pass (no store of the final state, no extra read)
static bool fuses_expval(const qmle_plan *plan, int meas_type) {
  return meas_type == QMLE_MEAS_EXPVAL_Z && !plan->stages.empty() && plan->stages.back().kind == ST_TILE;
}

// Which loop form a batch run of the executed plan takes in layout L (ChunkPipeline is built from the answer; no HIP
// call, no environment beyond what batch_layout read).  side: the side streams exist.
//   one_stream  one slot (one chunk, QMLE_NO_CHUNK_OVERLAP, QMLE_PLAN_NO_FUSION, no room, no side streams), or the
//               whole state in the LDS
//   staged      chunks that are filled one by one
//   alone       slots that stay zeroed, a measuring launch that streams at least 1 GiB -- route_tile's threshold for
//               the non-temporal policy: such a pass runs at the HBM's rate, and two of them at once lose 2-3 % to the
//               mix -- and at least four chunks: each slot is used twice, and every first pass from
//               chunk 2 on is queued while a measuring pass runs
//   free        the other runs whose slots stay zeroed (and staged runs of more stages than there are events)
static int chunk_loop_form(const qmle_plan *plan, int batch, int meas_type, const BatchLayout &L, bool side) {
  if (L.in_lds || L.slots != 2 || !side) return kChunkLoopOneStream;
  if (!slot_stays_zeroed(plan, fuses_expval(plan, meas_type)))
    return plan->stages.size() <= (size_t)kPipeStages ? kChunkLoopStaged : kChunkLoopFree;
  const int chunks = (batch + L.in_flight - 1) / L.in_flight;
  const bool hbm_bound = launch_streams_past_caches((uint64_t)L.in_flight, plan->n);
  return hbm_bound && chunks >= 4 ? kChunkLoopAlone : kChunkLoopFree;
}

static int run_batch_chunks(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                            const uint32_t *obs_masks, int n_obs, void *d_out, void *d_workspace,
                            size_t workspace_bytes, hipStream_t caller_stream, uint64_t token_in, uint64_t *token_out);

// The workspace token of qmle_run_batch_w (include/qmle_sv.h): what a call that returned QMLE_OK tells the next call
// on the same workspace about the zeros it left in the slots.  Bits 0..1 / 2..3: how many states of slot 0 / 1 hold
// zeros outside tile 0 of stage 0 -- 0 none, 1 a whole chunk (L.in_flight), 2 the batch's short last chunk -- the only
// counts a run's fills leave behind.  Bits 4..63: a fingerprint of everything that decides where those zeros lie and
// whether anything behind stage 0 stores into a slot: the schedule (every stage's kind and tile placement, the chosen
// candidate and padding, how often qmle_plan_autotune re-scheduled the plan), n, batch, measurement, the fill rule, the
// chunk size, the slots and where they start, the size and the address of the aligned workspace.  The engine keeps
// nothing: a token that does not carry the fingerprint of the call it is handed to counts as 0, and a run that leaves
// no zeros behind (every run that fills chunk by chunk, the whole-state-in-LDS runs) answers 0.
static uint64_t ws_fingerprint(const qmle_plan *plan, int batch, int meas_type, bool reuse_zeros, const BatchLayout &L,
                               const char *ws, size_t ws_bytes) {
  uint64_t h = fnv1a(&plan->n, sizeof(int));
  for (const Stage &st : plan->stages) {
    const int v[3] = {(int)st.kind, st.T, st.shift ? 1 : 0};
    h = fnv1a(v, sizeof(v), h);
    if (st.kind == ST_TILE) h = fnv1a(st.tile_bits, (size_t)st.T * sizeof(st.tile_bits[0]), h);
  }
  const uint64_t v[] = {(uint64_t)plan->chosen_candidate, (uint64_t)plan->pad_high, plan->schedule_serial,
                        plan->mat_floats, plan->flags, (uint64_t)batch, (uint64_t)meas_type, reuse_zeros ? 1u : 0u,
                        (uint64_t)L.in_flight, (uint64_t)L.slots, L.states[0], L.states[1], ws_bytes,
                        (uint64_t)(uintptr_t)ws};
  return (fnv1a(v, sizeof(v), h) << 4) | 16u;  // (never 0)
}
static int ws_token_states(uint64_t code, int batch, const BatchLayout &L) {
  return code == 1 ? L.in_flight : code == 2 ? batch % L.in_flight : 0;
}
static uint64_t ws_token_code(int zeroed, int batch, const BatchLayout &L) {
  return zeroed <= 0 ? 0u : zeroed == L.in_flight ? 1u : zeroed == batch % L.in_flight ? 2u : 0u;
}

// Simulate + measure; <Z> observables arrive as bit-position parity masks.  ws_token: qmle_run_batch_w's (may be NULL).
int qmle::run_batch_masks(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                          const uint32_t *obs_masks, int n_obs, void *d_out, void *d_workspace,
                          size_t workspace_bytes, hipStream_t caller_stream, uint64_t *ws_token) {
  const uint64_t token_in = ws_token ? *ws_token : 0;
  uint64_t token_out = 0;
  const int rc = run_batch_chunks(plan, d_angles, batch, meas_type, obs_masks, n_obs, d_out, d_workspace,
                                  workspace_bytes, caller_stream, token_in, &token_out);
  if (ws_token) *ws_token = rc == QMLE_OK ? token_out : 0;
  return rc;
}

// The chunks of a batch run whose states are resident in HBM: what the run's chunks share, and a chunk as three issue
// functions -- first pass, measuring pass, epilogue -- each of which takes its stream, and what it waits for, from the
// pipeline (ChunkPipeline::Part).  run_batch_chunks calls them chunk by chunk, or one chunk ahead with the first passes.
struct ChunkRun {
  qmle_plan *plan;
  const ChunkPipeline &pipe;
  const BatchLayout &L;
  const ObsClass &oc;
  const float *d_angles;
  int batch, meas_type;
  const uint32_t *obs_masks;
  int n_obs;
  void *d_out;
  char *ws;
  float *d_mats;
  float2 *d_cols;
  float *d_coef;
  const bool fuse_expval = fuses_expval(plan, meas_type);
  const bool fuse_mw = meas_type == QMLE_MEAS_MEYER_WALLACH && plan_mw_fusable(plan);
  const bool by_position = oc.single_bits || oc.semi_single;
  const bool reuse_zeros = slot_stays_zeroed(plan, fuse_expval);
  int slot_zeroed[2] = {0, 0};  // states of slot k that hold zeros outside tile 0 of stage 0
  uint64_t filled_states = 0;   // states written by fills, all chunks
  bool elided = false;          // a chunk ran without its fill

  struct Chunk {
    int no, b0, bc, slot;
    float2 *stc;
    void *d_partial;
    const float *mats, *ang;
    float2 *cols;
    bool initialised;
    TileRoute route;  // of the chunk's latest tile pass
  };
  Chunk chunk(int i) const {
    Chunk c;
    c.no = i;
    c.b0 = i * L.in_flight;
    c.bc = std::min(batch - c.b0, L.in_flight);
    c.slot = pipe.slot(i);
    const size_t D = (size_t)1 << plan->n;
    c.stc = meas_type == QMLE_MEAS_STATE ? (float2 *)d_out + (size_t)c.b0 * D : (float2 *)(ws + L.states[c.slot]);
    c.d_partial = ws + L.partial[c.slot];
    c.mats = d_mats + (size_t)c.b0 * plan->mat_floats;
    c.ang = d_angles ? d_angles + (size_t)c.b0 * plan->n_slots : nullptr;
    c.cols = d_cols ? d_cols + (size_t)c.b0 * plan->fold_groups * 16 : nullptr;
    c.initialised = false;
    return c;
  }

  int stage(Chunk &c, size_t si, hipStream_t stream) {
    const Stage &st = plan->stages[si];
    const ChunkPipeline::Queued stage_queued = pipe.begin_stage(c.no, si, stream);
    ProfScope prof_scope(plan, (int)si, stream);
    if (st.kind != ST_TILE) {
      if (!c.initialised) {
        launch_init_zero(c.stc, plan->n, c.bc, stream);
        c.initialised = true;
      }
      return run_stage_inplace(plan, st, c.stc, c.mats, c.ang, c.bc, stream);
    }
    const bool last = si + 1 == plan->stages.size();
    // the last pass stores the state AND reports its tile's Meyer-Wallach sums (one row per tile), or measures
    // <Z> instead of storing
    const bool last_mw = fuse_mw && last, last_fused = !fuse_mw && fuse_expval && last;
    const TileBuffers tb{c.stc, c.mats, c.ang, last_mw || last_fused ? c.d_partial : nullptr,
                         last_fused ? obs_masks : nullptr, c.cols, d_coef + (size_t)c.b0 * 32};
    TileRequest rq;
    rq.batch = c.bc;
    rq.init_zero = !c.initialised;
    rq.meas = last_mw ? TM_STORE_MW : !last_fused ? TM_STORE : by_position ? TM_EXPVAL_PARTIAL : TM_EXPVAL_MASKS;
    rq.n_obs = last_fused ? n_obs : 0;
    rq.from_zero = true;
    rq.fold_cols = c.cols != nullptr;
    rq.multi_rows = last_mw || (last_fused && (oc.single_bits || rq.meas == TM_EXPVAL_MASKS));
    rq.semi_single = oc.semi_single;
    const bool reuse = !last_mw && si == 0 && reuse_zeros;
    if (reuse) rq.zeroed_states = slot_zeroed[c.slot];
    const int rc = launch_tile(plan, si, tb, rq, stream, &c.route);
    note_product_form(plan, si, c.route, meas_type);
    if (last_fused && !is_reg_measure(c.route.family)) {  // (k_reg_measure* is no tile walk: the report stays "no such pass")
      plan->last_run.measure_tpw = 1 << c.route.row_shift;
      plan->last_run.measure_regs = c.route.from_regs;
      plan->last_run.wave_private = c.route.wave_private;
      plan->last_run.staging_dma = (c.route.walk & kWalkDma) != 0;
      plan->last_run.lane_swap = (c.route.walk & kWalkLaneSwap) != 0;
      plan->last_run.walk_kernel = c.route.walk_kernel;
    }
    if (reuse && c.route.fill) {
      slot_zeroed[c.slot] = c.bc;
      filled_states += (uint64_t)c.bc;
    }
    if (reuse && c.route.fill_elided) elided = true;
    c.initialised = true;
    return rc;
  }

  // stage 0, with the fill if launch_tile asks for one
  int first_pass(Chunk &c) {
    if (plan->stages.empty()) return QMLE_OK;
    const ChunkPipeline::Queued queued = pipe.begin_part(c.no, ChunkPipeline::kFirst);
    return stage(c, 0, queued.stream);
  }
  // the stages behind it; of a run whose slots stay zeroed, the measuring pass
  int measuring_pass(Chunk &c) {
    const ChunkPipeline::Queued queued = pipe.begin_part(c.no, ChunkPipeline::kMeasure);
    for (size_t si = 1; si < plan->stages.size(); ++si) {
      const int rc = stage(c, si, queued.stream);
      if (rc != QMLE_OK) return rc;
    }
    return QMLE_OK;
  }
  // measure the chunk
  int epilogue(Chunk &c) {
    const ChunkPipeline::Queued queued = pipe.begin_part(c.no, ChunkPipeline::kEpilogue);
    const hipStream_t stream = queued.stream;
    const int n = plan->n;
    const size_t D = (size_t)1 << n;
    int rc = QMLE_OK;
    if (!c.initialised) launch_init_zero(c.stc, n, c.bc, stream);
    if (meas_type == QMLE_MEAS_PROBS) {
      const uint64_t tc = (uint64_t)c.bc * (D / 2);
      launch_probs(c.stc, (float *)d_out + (size_t)c.b0 * D, tc, stream);
    } else if (meas_type == QMLE_MEAS_EXPVAL_Z && fuse_expval) {
      // column of the 33-float row: the bit's sum, or (masks, k_reg_measure) the observable's own
      const bool reg_measure = is_reg_measure(c.route.family);
      const int tiles = (1 << (n - plan->stages.back().T)) >> c.route.row_shift;
      launch_expval_final((const float *)c.d_partial, tiles, c.bc, n_obs,
                          by_position && !reg_measure ? oc.by_position : oc.by_index,
                          (float *)d_out + (size_t)c.b0 * n_obs, stream);
    } else if (meas_type == QMLE_MEAS_EXPVAL_Z) {
      rc = oc.single_bits
               ? run_expval(c.stc, n, c.bc, oc.by_position.bits, n_obs, (float *)d_out + (size_t)c.b0 * n_obs,
                            c.d_partial, L.partial_bytes, stream)
               : run_parity_pos(c.stc, n, c.bc, obs_masks, n_obs, (float *)d_out + (size_t)c.b0 * n_obs,
                                c.d_partial, L.partial_bytes, stream);
      if (rc != QMLE_OK) return rc;
    } else if (meas_type == QMLE_MEAS_MEYER_WALLACH) {
      rc = fuse_mw ? run_mw_fused(c.stc, n, c.bc, plan->stages.back(), c.route.row_shift, c.d_partial, L.partial_bytes,
                                  (float *)d_out + (size_t)c.b0 * (n + 1), stream, &plan->last_run.mw_finish)
                   : run_mw_resident(c.stc, n, c.bc, c.d_partial, L.partial_bytes,
                                     (float *)d_out + (size_t)c.b0 * (n + 1), stream);
      if (rc != QMLE_OK) return rc;
    } else if (meas_type == QMLE_MEAS_DENSITY) {
      if (n > 15) return QMLE_ERR_UNSUPPORTED;
      launch_density(c.stc, (float2 *)d_out + (size_t)c.b0 * D * D, n, c.bc, stream);
    }
    HIPCHK(hipGetLastError());
    return QMLE_OK;
  }
};

static int run_batch_chunks(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                            const uint32_t *obs_masks, int n_obs, void *d_out, void *d_workspace,
                            size_t workspace_bytes, hipStream_t caller_stream, uint64_t token_in, uint64_t *token_out) {
  if (plan->zero_variant) plan = plan->zero_variant;  // every run_batch starts from |0..0>
  plan->last_run = LastRun();  // (a run that fails reports the fresh-buffer figure and no measuring pass)
  const int n = plan->n;
  ObsClass oc;
  if (meas_type == QMLE_MEAS_EXPVAL_Z) oc = classify_observables(plan, obs_masks, n_obs);
  int rc = ensure_device_plan(plan);
  if (rc != QMLE_OK) return rc;

  char *ws = (char *)d_workspace;
  BatchLayout L;
  if (!align_workspace(ws, workspace_bytes) || !batch_layout(plan, batch, meas_type, 0, &workspace_bytes, L))
    return QMLE_ERR_WORKSPACE;
  float *d_mats = (float *)ws;
  float2 *d_cols = plan->fold_groups ? (float2 *)(ws + L.cols) : nullptr;
  float *d_coef = (float *)(ws + L.coef);

  // per-sample gate matrices for the whole batch (tiny)
  // (the records of the last stage's closing-free groups: without closing diagonals when the run ends in |amplitude|^2)
  const uint32_t measured_from = measured_records_from(plan, meas_type);
  rc = launch_build_matrices(plan, d_angles, d_mats, batch, caller_stream, /*forward_only=*/true, measured_from);
  if (rc != QMLE_OK) return rc;
  plan->last_run.matrices_from_map = plan->n_groups_needed > 0 && qmle::builds_from_map(batch);
  plan->last_run.chunk_loop = kChunkLoopOneStream;
  if (L.in_lds)
    return run_batch_lds(plan, L, d_mats, d_angles, batch, meas_type, obs_masks, n_obs, d_out, ws + L.partial[0],
                         caller_stream);

  // ---- general path: states resident in HBM, sample-major chunks ----------------
  ChunkPipeline pipe(chunk_loop_form(plan, batch, meas_type, L, /*side=*/L.slots == 2), caller_stream);
  plan->last_run.chunk_loop = pipe.form();
  ChunkRun run{plan, pipe, L, oc, d_angles, batch, meas_type, obs_masks, n_obs, d_out, ws, d_mats, d_cols, d_coef};
  const bool reuse_zeros = run.reuse_zeros;
  // Clean slots: slot_zeroed[k] states of slot k hold zeros outside tile 0 of stage 0.  The caller owns the workspace
  // between calls, so a slot's first chunk is filled -- unless the caller hands back the token of the call before
  // (qmle_run_batch_w: nobody wrote the workspace since, and this call is ordered behind that one) and the token carries
  // this call's fingerprint: then the slots start as that call left them.  A slot's first passes are queued in chunk
  // order on one stream, and each behind the slot's measuring pass before it, whichever loop form this is.
  const uint64_t fingerprint = ws_fingerprint(plan, batch, meas_type, reuse_zeros, L, ws, workspace_bytes);
  if (reuse_zeros && (token_in & ~(uint64_t)15) == fingerprint)
    for (int k = 0; k < L.slots; ++k) run.slot_zeroed[k] = ws_token_states((token_in >> (2 * k)) & 3u, batch, L);
  const int chunks = (batch + L.in_flight - 1) / L.in_flight;
  if (pipe.form() == kChunkLoopAlone) {
    // one chunk ahead on the stream of the first passes (ChunkPipeline)
    ChunkRun::Chunk cur = run.chunk(0), next = cur;
    rc = run.first_pass(cur);
    for (int i = 0; i < chunks && rc == QMLE_OK; ++i, cur = next) {
      if (i + 1 < chunks) {
        next = run.chunk(i + 1);
        rc = run.first_pass(next);
      }
      if (rc == QMLE_OK) rc = run.measuring_pass(cur);
      if (rc == QMLE_OK) rc = run.epilogue(cur);
    }
  } else {
    for (int i = 0; i < chunks && rc == QMLE_OK; ++i) {
      ChunkRun::Chunk c = run.chunk(i);
      rc = run.first_pass(c);
      if (rc == QMLE_OK) rc = run.measuring_pass(c);
      if (rc == QMLE_OK) rc = run.epilogue(c);
    }
  }
  if (rc != QMLE_OK) return rc;
  // what qmle_plan_describe reports as stage 0's written bytes (a report: nothing in the engine reads it): the fills
  // and tile-0 stores of this run per state when fills were left out, else 0 = the fresh-buffer figure
  if (run.elided)
    plan->last_run.stage0_written =
        ((run.filled_states << (n + 3)) + ((uint64_t)batch << (plan->stages[0].T + 3))) / (uint64_t)batch;
  uint64_t codes = 0;
  if (reuse_zeros)
    for (int k = 0; k < L.slots; ++k) codes |= ws_token_code(run.slot_zeroed[k], batch, L) << (2 * k);
  *token_out = codes ? fingerprint | codes : 0;  // (no zeros to hand on: no token)
  return QMLE_OK;
}

// chunk_loop_form for a 256-byte-aligned workspace of the size the query answers, given that the side streams exist
const char *qmle_chunk_loop_form(const qmle_plan *plan, int batch, int meas_type, int states_in_flight) {
  if (!plan || batch < 1 || meas_type < QMLE_MEAS_STATE || meas_type > QMLE_MEAS_MEYER_WALLACH)
    return kChunkLoopNames[kChunkLoopNone];
  const size_t bytes = qmle_workspace_bytes(plan, batch, meas_type, 0, states_in_flight);
  const qmle_plan *exec = qmle_plan_executed(const_cast<qmle_plan *>(plan), meas_type);
  BatchLayout L;
  if (!batch_layout(exec, batch, meas_type, 0, &bytes, L, /*side=*/1)) return kChunkLoopNames[kChunkLoopNone];
  return kChunkLoopNames[chunk_loop_form(exec, batch, meas_type, L, /*side=*/true)];
}

// Apply the plan's passes IN PLACE to resident states (no |0..0> initialisation, no
// measurement): the gate-application hot loop on its own (simulation.py:102-103).
// One stage of a plan applied in place to resident states.
int qmle::run_stage_inplace(qmle_plan *plan, const Stage &st, float2 *d_states, const float *d_mats,
                            const float *d_angles, int batch, hipStream_t stream) {
  if (st.kind == ST_TILE) {
    const size_t si = (size_t)(&st - plan->stages.data());
    const TileBuffers tb{d_states, d_mats, d_angles};
    TileRequest rq;
    rq.batch = batch;
    TileRoute route;
    const int rc = launch_tile(plan, si, tb, rq, stream, &route);
    note_product_form(plan, si, route);
    return rc;
  }
  if (st.kind == ST_DIRECT)
    return launch_direct(plan, plan->dev_ops[st.op_begin], d_states, d_mats, batch, stream);
  const LoweredOp &o = plan->dev_ops[st.op_begin];
  launch_diag_all(d_states, plan->n, batch, plan->dev.d_consts + o.mat_off, d_angles, plan->n_slots, o.slot, stream);
  return QMLE_OK;
}

int qmle_apply_inplace(qmle_plan *plan, const float *d_angles, int batch, void *d_states,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream_) {
  if (!plan || batch < 1 || batch > kMaxGridY || !d_states || !d_workspace) return QMLE_ERR_INVALID_ARG;
  if (plan->n_slots > 0 && !d_angles) return QMLE_ERR_INVALID_ARG;
  // (a schedule compiled for runs from |0..0> -- qmle_plan_executed's handle -- is not one for live states)
  if (plan->flags & QMLE_PLAN_INTERNAL_ZERO_RUN) return QMLE_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  int rc = ensure_device_plan(plan);
  if (rc != QMLE_OK) return rc;
  char *ws = (char *)d_workspace;
  if (!align_workspace(ws, workspace_bytes) || workspace_bytes < ws_mats_bytes(plan, batch)) return QMLE_ERR_WORKSPACE;
  float *d_mats = (float *)ws;
  rc = launch_build_matrices(plan, d_angles, d_mats, batch, stream, /*forward_only=*/true);
  if (rc != QMLE_OK) return rc;
  int stage_idx = -1;
  for (const Stage &st : plan->stages) {
    ProfScope prof_scope(plan, ++stage_idx, stream);
    rc = run_stage_inplace(plan, st, (float2 *)d_states, d_mats, d_angles, batch, stream);
    if (rc != QMLE_OK) return rc;
  }
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}


// ---- plan autotuner (opt-in; the default schedule stays the cost model's, deterministically) ----------
// The pass-cost model ranks the schedule candidates from measurements at n = 24; which positions share a
// tile moves a pass by up to +-20 % through an address hash nobody documents, and away from
// n = 24 the model's favourite is sometimes 5-7 % off the best.  qmle_plan_autotune times the model's best
// `top_k` candidates (x the two paddings of the last stage) ON THE DEVICE with the caller's batch size and
// measurement, and re-schedules the plan that qmle_run_batch executes to the fastest.  Every candidate is
// the same tape under another order of commuting gates / another tile geometry: results equal to float32
// rounding (tests/test_gpu_kernels.py runs every one of them).  Choices are remembered per (tape, flags, device).
namespace {

struct TunedChoice { int cand, pad; };
static std::mutex g_tuned_mu;
static std::map<uint64_t, TunedChoice> g_tuned;

static uint64_t tape_hash(const qmle_plan *p, int meas_class, int batch_class) {
  const int v[6] = {p->n, p->n_slots, (int)p->flags, meas_class, batch_class, current_device()};
  return fnv1a(v, sizeof(v), fnv1a(p->ops.data(), p->ops.size() * sizeof(qmle_op)));
}

// a stand-alone compile of `base`'s tape with a forced candidate (no variant, no child)
static qmle_plan *compile_candidate(const qmle_plan *base, int cand, int pad) {
  qmle_plan *c = new_plan_like(base, base->ops, base->flags);
  if (!c) return nullptr;
  c->force_candidate = cand;
  c->pad_high = pad;
  c->extra_algo_last_stage = base->extra_algo_last_stage;
  if (compile_plan(c) != QMLE_OK || c->chosen_candidate != cand) {
    (void)qmle_plan_destroy(c);
    return nullptr;
  }
  return c;
}

static bool same_stages(const qmle_plan *a, const qmle_plan *b) {
  if (a->stages.size() != b->stages.size()) return false;
  for (size_t s = 0; s < a->stages.size(); ++s)
    if (a->stages[s].T != b->stages[s].T || a->stages[s].kind != b->stages[s].kind ||
        std::memcmp(a->stages[s].tile_bits, b->stages[s].tile_bits, (size_t)a->stages[s].T) != 0 ||
        a->stages[s].op_end - a->stages[s].op_begin != b->stages[s].op_end - b->stages[s].op_begin)
      return false;
  return true;
}

// dst keeps its identity (handles, children, folded tail); its schedule becomes src's
static void adopt_schedule(qmle_plan *dst, qmle_plan *src) {
  if (dst->dev.blob) { (void)hipFree(dst->dev.blob); dst->dev = DevicePlan(); }
  if (dst->f64_blob) { (void)hipFree(dst->f64_blob); dst->f64_blob = nullptr; dst->f64_device = -1; }
  dst->consts.swap(src->consts);
  dst->lowered.swap(src->lowered);
  dst->lowered_src.swap(src->lowered_src);
  dst->dev_ops.swap(src->dev_ops);
  dst->dev_src.swap(src->dev_src);
  dst->op_groups.swap(src->op_groups);
  dst->ops2.swap(src->ops2);
  dst->groups2.swap(src->groups2);
  dst->tbl2.swap(src->tbl2);
  dst->build_ops.swap(src->build_ops);
  dst->groups.swap(src->groups);
  dst->stages.swap(src->stages);
  dst->cand_ranking.swap(src->cand_ranking);
  std::swap(dst->mat_floats, src->mat_floats);
  std::swap(dst->mat_floats_old, src->mat_floats_old);
  std::swap(dst->mat_floats_unit, src->mat_floats_unit);
  std::swap(dst->n_groups_needed, src->n_groups_needed);
  std::swap(dst->n_product_groups, src->n_product_groups);
  std::swap(dst->fold_groups, src->fold_groups);
  std::swap(dst->model_cost, src->model_cost);
  std::swap(dst->chosen_candidate, src->chosen_candidate);
  std::swap(dst->whole_state_lds, src->whole_state_lds);
  std::swap(dst->tile_T, src->tile_T);
  std::swap(dst->tile_L, src->tile_L);
  std::swap(dst->algo_bytes_per_state, src->algo_bytes_per_state);
  dst->force_candidate = src->force_candidate;
  dst->pad_high = src->pad_high;
  dst->last_run.stage0_written = 0;  // (the figure of a run of the old schedule)
  dst->schedule_serial++;            // (... and so are the zeros a run of it left in a workspace: ws_fingerprint)
  dst->autotuned = true;
}

}  // namespace

int qmle_plan_autotune(qmle_plan *plan, int meas_type, int n_obs, int batch, int top_k, int reps,
                       qmle_stream stream_, int32_t *chosen, double *ms_before, double *ms_after) {
  if (!plan || batch < 1 || top_k < 1 || reps < 1) return QMLE_ERR_INVALID_ARG;
  if (meas_type != QMLE_MEAS_STATE && meas_type != QMLE_MEAS_EXPVAL_Z) return QMLE_ERR_MEAS_TYPE;
  if (meas_type == QMLE_MEAS_EXPVAL_Z && (n_obs < 1 || n_obs > plan->n)) return QMLE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (chosen) { chosen[0] = chosen[1] = -1; }
  if (ms_before) *ms_before = 0.0;
  if (ms_after) *ms_after = 0.0;
  // the plan this measurement executes
  qmle_plan *owner = (meas_type == QMLE_MEAS_EXPVAL_Z && plan->expval_child) ? plan->expval_child : plan;
  qmle_plan *target = owner->zero_variant ? owner->zero_variant : owner;
  if (target->whole_state_lds || target->cand_ranking.size() < 2 || (target->flags & QMLE_PLAN_NO_FUSION) ||
      ((target->flags >> 8) & 0xffffu))
    return QMLE_OK;  // one schedule only: nothing to tune
  const int batch_class = batch >= 256 ? 2 : batch >= 16 ? 1 : 0;
  // keyed by the TARGET plan, not by the measurement: without a folded child "state" and "expval" execute the
  // same plan, and two remembered choices for one plan would overwrite each other's schedule (and rebuild the
  // device image) on every alternation.  The first measurement tuned decides; the other adopts its choice.
  const uint64_t key = tape_hash(target, owner != plan ? 1 : 0, batch_class);
  {
    std::lock_guard<std::mutex> lock(g_tuned_mu);
    auto it = g_tuned.find(key);
    if (it != g_tuned.end()) {  // tuned before in this process: adopt the remembered choice, no timing
      if (it->second.cand != target->chosen_candidate || it->second.pad != (target->pad_high > 0 ? 1 : 0)) {
        qmle_plan *c = compile_candidate(target, it->second.cand, it->second.pad);
        if (c) { adopt_schedule(target, c); (void)qmle_plan_destroy(c); }
      }
      target->autotuned = true;
      if (chosen) { chosen[0] = target->chosen_candidate; chosen[1] = target->pad_high > 0 ? 1 : 0; }
      return QMLE_OK;
    }
  }
  // scratch of this one-off step: a zero angle table, the output and a workspace large enough for every candidate
  const int n = target->n;
  const size_t D = (size_t)1 << n;
  const size_t ang_bytes = (size_t)batch * (target->n_slots ? target->n_slots : 1) * sizeof(float);
  const size_t out_bytes = meas_type == QMLE_MEAS_STATE ? (size_t)batch * D * sizeof(float2) : (size_t)batch * n_obs * sizeof(float);
  uint32_t masks[QMLE_MAX_QUBITS];
  for (int k = 0; k < QMLE_MAX_QUBITS; ++k) masks[k] = 1u << (k < n ? k : 0);
  struct Cand { qmle_plan *p; int cand, pad; double ms; };
  std::vector<Cand> cands;
  cands.push_back({nullptr, target->chosen_candidate, target->pad_high > 0 ? 1 : 0, 0.0});  // the current schedule, as it stands
  for (size_t i = 0; i < target->cand_ranking.size() && (int)i < top_k; ++i)
    for (int pad = 0; pad < 2; ++pad) {
      const int k = target->cand_ranking[i].second;
      if (k == cands[0].cand && pad == cands[0].pad) continue;
      qmle_plan *c = compile_candidate(target, k, pad);
      if (!c) continue;
      // (a padding that changes nothing compiles to the same stages: skip the duplicate)
      bool dup = false;
      for (const Cand &o : cands)
        if (o.cand == k && same_stages(o.p ? o.p : target, c)) dup = true;
      if (dup) { (void)qmle_plan_destroy(c); continue; }
      cands.push_back({c, k, pad, 0.0});
    }
  size_t ws_bytes = workspace_bytes_one(target, batch, meas_type, 0);
  for (const Cand &c : cands)
    if (c.p) ws_bytes = std::max(ws_bytes, workspace_bytes_one(c.p, batch, meas_type, 0));
  char *scratch = nullptr;
  const size_t total = align_up(ang_bytes, 256) + align_up(out_bytes, 256) + ws_bytes + 512;
  if (hipMalloc((void **)&scratch, total) != hipSuccess) {
    for (Cand &c : cands) if (c.p) (void)qmle_plan_destroy(c.p);
    (void)hipGetLastError();
    if (chosen) chosen[1] = -2;  // "not tuned" (as opposed to -1 / -1: nothing to tune): the caller may try again
    return QMLE_OK;  // no room to tune next to the caller's buffers: keep the model's schedule
  }
  float *d_ang = (float *)scratch;
  void *d_out = scratch + align_up(ang_bytes, 256);
  void *d_ws = scratch + align_up(ang_bytes, 256) + align_up(out_bytes, 256);
  int rc = QMLE_OK;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipMemsetAsync(d_ang, 0, ang_bytes, stream) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
      hipEventCreate(&e1) != hipSuccess)
    rc = QMLE_ERR_HIP;
  for (size_t i = 0; i < cands.size() && rc == QMLE_OK; ++i) {
    qmle_plan *run = cands[i].p ? cands[i].p : target;
    for (int r = -1; r < reps && rc == QMLE_OK; ++r) {  // r = -1: warm-up (device image upload, attributes)
      if (r == 0) (void)hipEventRecord(e0, stream);
      rc = run_batch_masks(run, d_ang, batch, meas_type, masks, n_obs, d_out, d_ws, ws_bytes, stream);
    }
    if (rc != QMLE_OK) break;
    (void)hipEventRecord(e1, stream);
    if (hipEventSynchronize(e1) != hipSuccess) { rc = QMLE_ERR_HIP; break; }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    cands[i].ms = (double)ms / reps;
  }
  size_t best = 0;
  if (rc == QMLE_OK) {
    for (size_t i = 1; i < cands.size(); ++i)
      if (cands[i].ms < cands[best].ms * 0.99) best = i;  // (a candidate must win by 1 %: ties keep the model's choice)
    if (ms_before) *ms_before = cands[0].ms;
    if (ms_after) *ms_after = cands[best].ms;
    if (best != 0) adopt_schedule(target, cands[best].p);
    target->autotuned = true;
    if (chosen) { chosen[0] = cands[best].cand; chosen[1] = cands[best].pad; }
    std::lock_guard<std::mutex> lock(g_tuned_mu);
    g_tuned[key] = {cands[best].cand, cands[best].pad};
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipStreamSynchronize(stream);
  (void)hipFree(scratch);
  for (Cand &c : cands) if (c.p) (void)qmle_plan_destroy(c.p);
  return rc;
}

// the ABI's leaf arrays -> the kernels' AngleLeaves (the caller has checked 0 <= n_leaves <= 8)
static int fill_angle_leaves(AngleLeaves &lv, const float *const *d_leaves, const int64_t *leaf_strides,
                             const int32_t *leaf_div, const int32_t *leaf_mod, int n_leaves) {
  std::memset(&lv, 0, sizeof(lv));
  for (int k = 0; k < n_leaves; ++k) {
    // (a leaf without elements -- the parameters of an ansatz that has none -- may come as a NULL pointer: no term can refer to it)
    if ((!d_leaves[k] && leaf_strides[k] != 0) || leaf_div[k] < 1 || leaf_mod[k] < 1) return QMLE_ERR_INVALID_ARG;
    lv.ptr[k] = d_leaves[k];
    lv.stride[k] = leaf_strides[k];
    lv.div[k] = leaf_div[k];
    lv.mod[k] = leaf_mod[k];
  }
  return QMLE_OK;
}

int qmle_build_angles(const float *const *d_leaves, const int64_t *leaf_strides,
                      const int32_t *leaf_div, const int32_t *leaf_mod, int n_leaves,
                      const int32_t *d_ptr, const int32_t *d_arg, const int32_t *d_idx,
                      const float *d_coef, const float *d_const, const double *d_period,
                      int n_slots, int64_t batch, int64_t batch_offset, float *d_out,
                      qmle_stream stream) {
  // (a negative offset would wrap as an unsigned row)
  if (n_leaves < 0 || n_leaves > 8 || n_slots < 0 || batch < 1 || batch_offset < 0 || !d_out || !d_ptr || !d_const)
    return QMLE_ERR_INVALID_ARG;
  if (n_slots == 0) return QMLE_OK;
  AngleLeaves lv;
  const int rc_lv = fill_angle_leaves(lv, d_leaves, leaf_strides, leaf_div, leaf_mod, n_leaves);
  if (rc_lv != QMLE_OK) return rc_lv;
  const uint64_t total = (uint64_t)batch * (uint64_t)n_slots;
  if (total + 256 < (1ull << 32) && (uint64_t)batch + (uint64_t)batch_offset < (1ull << 32))
    hipLaunchKernelGGL(k_build_angles<uint32_t>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, lv,
                       d_ptr, d_arg, d_idx, d_coef, d_const, d_period, n_slots, (long long)batch,
                       (long long)batch_offset, d_out);
  else
    hipLaunchKernelGGL(k_build_angles<unsigned long long>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       lv, d_ptr, d_arg, d_idx, d_coef, d_const, d_period, n_slots, (long long)batch,
                       (long long)batch_offset, d_out);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

int qmle_run_batch_map(qmle_plan *plan, const qmle_angle_map *map, float *d_angles, int batch,
                       int meas_type, const int32_t *obs_wires, int n_obs, void *d_out,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream) {
  return qmle_run_batch_map_w(plan, map, d_angles, batch, meas_type, obs_wires, n_obs, d_out, d_workspace,
                              workspace_bytes, stream, nullptr);
}

int qmle_run_batch_map_w(qmle_plan *plan, const qmle_angle_map *map, float *d_angles, int batch,
                         int meas_type, const int32_t *obs_wires, int n_obs, void *d_out,
                         void *d_workspace, size_t workspace_bytes, qmle_stream stream, uint64_t *ws_token) {
  if (!plan || !map || batch < 1 || map->batch_offset < 0) return void_token(ws_token, QMLE_ERR_INVALID_ARG);
  if (plan->n_slots == 0)
    return qmle_run_batch_w(plan, d_angles, batch, meas_type, obs_wires, n_obs, d_out, d_workspace, workspace_bytes,
                            stream, ws_token);
  if (!d_angles) return void_token(ws_token, QMLE_ERR_INVALID_ARG);
  // The table is needed as a table only by the Golomb diagonal (QMLE_OP_DIAG_ALL reads its angle in the pass
  // itself); every other gate meets its angles in the matrix builder, which can form them from the map --
  // one kernel (5-9 us of the 0.17 ms analysis loops) and the table's round trip less.  From 64 samples on
  // (whole waves per group).
  bool table = batch < 64 || map->n_leaves < 0 || map->n_leaves > 8 || !map->d_ptr || !map->d_const;
  for (const qmle_op &o : plan->ops) table = table || o.opcode == QMLE_OP_DIAG_ALL;
  if (table) {
    const int rc = qmle_build_angles(map->d_leaves, map->leaf_strides, map->leaf_div, map->leaf_mod, map->n_leaves,
                                     map->d_ptr, map->d_arg, map->d_idx, map->d_coef, map->d_const, map->d_period,
                                     plan->n_slots, batch, map->batch_offset, d_angles, stream);
    if (rc != QMLE_OK) return void_token(ws_token, rc);
    return qmle_run_batch_w(plan, d_angles, batch, meas_type, obs_wires, n_obs, d_out, d_workspace, workspace_bytes,
                            stream, ws_token);
  }
  AngleMapSrc src;
  std::memset(&src, 0, sizeof(src));
  const int rc_lv = fill_angle_leaves(src.lv, map->d_leaves, map->leaf_strides, map->leaf_div, map->leaf_mod, map->n_leaves);
  if (rc_lv != QMLE_OK) return void_token(ws_token, rc_lv);
  src.ptr = map->d_ptr; src.arg = map->d_arg; src.idx = map->d_idx;
  src.coef = map->d_coef; src.cst = map->d_const; src.period = map->d_period;
  src.b_offset = map->batch_offset;
  src.small = (uint64_t)batch + (uint64_t)map->batch_offset < (1ull << 32);
  tls_angle_map = &src;
  const int rc = qmle_run_batch_w(plan, d_angles, batch, meas_type, obs_wires, n_obs, d_out, d_workspace,
                                  workspace_bytes, stream, ws_token);
  tls_angle_map = nullptr;
  return rc;
}

int qmle_profile_begin(qmle_plan *plan, int capacity) {
  if (!plan || capacity < 1) return QMLE_ERR_INVALID_ARG;
  // (qmle_run_batch executes the from-|0..0> variant when there is one: its launches are the ones to time)
  if (plan->zero_variant) {
    const int rc = qmle_profile_begin(plan->zero_variant, capacity);
    if (rc != QMLE_OK) return rc;
  }
  StageProfile &pr = plan->prof;
  while ((int)pr.start.size() < capacity) {
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    pr.start.push_back((void *)a);
    pr.stop.push_back((void *)b);
  }
  pr.stage.assign(pr.start.size(), -1);
  pr.used = 0;
  pr.on = true;
  return QMLE_OK;
}

int qmle_profile_end(qmle_plan *plan, double *stage_ms, int64_t *stage_launches, int n_stages) {
  if (!plan || !stage_ms || !stage_launches) return QMLE_ERR_INVALID_ARG;
  if (plan->zero_variant && plan->zero_variant->prof.on) {
    // the variant ran (qmle_run_batch) unless the plan itself recorded launches (qmle_apply_inplace)
    if (plan->prof.used == 0) {
      plan->prof.on = false;
      for (size_t k = 0; k < plan->prof.start.size(); ++k) {
        (void)hipEventDestroy((hipEvent_t)plan->prof.start[k]);
        (void)hipEventDestroy((hipEvent_t)plan->prof.stop[k]);
      }
      plan->prof.start.clear(); plan->prof.stop.clear(); plan->prof.stage.clear();
      return qmle_profile_end(plan->zero_variant, stage_ms, stage_launches, n_stages);
    }
    std::vector<double> ms(plan->zero_variant->stages.size() + 1);
    std::vector<int64_t> cnt(plan->zero_variant->stages.size() + 1);
    (void)qmle_profile_end(plan->zero_variant, ms.data(), cnt.data(), (int)ms.size());
  }
  if (n_stages < (int)plan->stages.size()) return QMLE_ERR_INVALID_ARG;
  StageProfile &pr = plan->prof;
  pr.on = false;
  for (int i = 0; i < n_stages; ++i) { stage_ms[i] = 0.0; stage_launches[i] = 0; }
  for (size_t k = 0; k < pr.used; ++k) {
    HIPCHK(hipEventSynchronize((hipEvent_t)pr.stop[k]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, (hipEvent_t)pr.start[k], (hipEvent_t)pr.stop[k]));
    stage_ms[pr.stage[k]] += ms;
    stage_launches[pr.stage[k]] += 1;
  }
  const int dropped = pr.used >= pr.start.size() ? 1 : 0;
  for (size_t k = 0; k < pr.start.size(); ++k) {
    (void)hipEventDestroy((hipEvent_t)pr.start[k]);
    (void)hipEventDestroy((hipEvent_t)pr.stop[k]);
  }
  pr.start.clear(); pr.stop.clear(); pr.stage.clear(); pr.used = 0;
  return dropped;  // 1 = the pool filled up (later launches were not timed)
}

