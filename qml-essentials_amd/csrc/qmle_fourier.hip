// Analytic Fourier coefficients: the sine-cosine tree of a Pauli-rotation circuit, merged into a DAG and walked with
// numbers (qmle_fourier_dag; tables, recurrence and status codes in include/qmle_sv.h, design in DESIGN.md 6.14).
//
// Work split.  One workgroup of kFourierThreads lanes owns one sample.  It walks the levels in circuit order; inside a
// level its lanes are spread over the items (node of the level, grid point), item = node * F + g, so neighbouring lanes
// write neighbouring complex128 values and read neighbouring values of the (same or a neighbouring) child.  Between two
// levels stands a workgroup barrier: a level reads only values of lower levels, which the same workgroup stored through
// the same L1.  Every value has one writer, every sum is written out in a fixed order, there is no atomic: the output is
// bit-reproducible.  Many samples fill the card; one sample with a large DAG occupies one compute unit and is merely
// slow (no grid-wide barrier is built for it).
//
// Memory.  The values of a sample are its slice of the workspace, n_nodes x F complex128.  The sines and cosines of a
// sample's angles are evaluated once, on the device, by the lanes of its workgroup (one level each) and kept beside the
// values as n_levels x (cos, sin); a SHIFT level reads nothing there.
//
// Registers.  Per lane: the item counter, one node record (16 B), two or four child values and the result -- nothing is
// indexed at run time, the grid axis is a loop over memory.  No LDS, no scratch.
#include <vector>

#include "qmle_dev.h"

namespace {

constexpr int kFourierThreads = 256;

// a level as the kernel reads it: the axis of a SHIFT level is resolved into the stride and length of that axis
struct FourierLevel {
  int32_t node_begin, node_end, kind, column;
  int32_t shift, stride, dim, pad;
};

struct FourierLaunch {
  const qmle_fourier_node *nodes;
  const FourierLevel *levels;
  const int32_t *roots;       // n_roots children codes, then n_roots phases
  const double *angles;       // [batch][n_columns]
  double2 *trig;              // [batch][n_levels] (cos, sin)
  double2 *values;            // [batch][n_nodes][F]
  double2 *out;               // [batch][n_roots][F]
  int32_t n_nodes, n_levels, n_roots, n_columns, F, centre;
};

// i^k z, k in 0..3, without a branch
__device__ __forceinline__ double2 times_i_pow(double2 z, int k) {
  const double re = (k & 1) ? z.y : z.x;
  const double im = (k & 1) ? z.x : z.y;
  const double sr = (k == 1 || k == 2) ? -1.0 : 1.0;  // 1: (x, y)  i: (-y, x)  -1: (-x, -y)  -i: (y, -x)
  const double si = (k >= 2) ? -1.0 : 1.0;
  return make_double2(sr * re, si * im);
}

// the value of a child slot at grid point g: a node of a lower level, the unit at omega = 0, or zero
__device__ __forceinline__ double2 child_value(const double2 *V, int child, int F, int centre, int g) {
  if (child >= 0) return V[(size_t)child * (size_t)F + (size_t)g];
  return make_double2((child == QMLE_FOURIER_ONE && g == centre) ? 1.0 : 0.0, 0.0);
}

__global__ __launch_bounds__(kFourierThreads) void k_fourier_dag(FourierLaunch L) {
  const int b = blockIdx.x;
  const int F = L.F, centre = L.centre;
  double2 *V = L.values + (size_t)b * (size_t)L.n_nodes * (size_t)F;
  double2 *trig = L.trig + (size_t)b * (size_t)L.n_levels;
  const double *angles = L.angles + (size_t)b * (size_t)L.n_columns;

  for (int l = threadIdx.x; l < L.n_levels; l += kFourierThreads) {
    double s = 0.0, c = 1.0;
    if (L.levels[l].kind == QMLE_FOURIER_ANGLE && L.levels[l].node_end > L.levels[l].node_begin)
      sincos(angles[L.levels[l].column], &s, &c);
    trig[l] = make_double2(c, s);
  }
  __syncthreads();

  for (int l = 0; l < L.n_levels; ++l) {
    const FourierLevel lv = L.levels[l];  // the same record in every lane
    const int items = (lv.node_end - lv.node_begin) * F;
    if (items == 0) continue;  // (uniform: every lane skips the barrier of an empty level)
    if (lv.kind == QMLE_FOURIER_ANGLE && F == 1) {
      // plain numbers (FourierTree.__call__: every level is an ANGLE): item = node, no division by the grid size
      const double2 cs = trig[l];
      for (int it = threadIdx.x; it < items; it += kFourierThreads) {
        const int node = lv.node_begin + it;
        const qmle_fourier_node nd = L.nodes[node];
        const double2 a = child_value(V, nd.cos_child, 1, centre, 0);
        const double2 sb = times_i_pow(child_value(V, nd.sin_child, 1, centre, 0), (nd.power + 1) & 3);
        V[node] = make_double2(cs.x * a.x + cs.y * sb.x, cs.x * a.y + cs.y * sb.y);
      }
    } else if (lv.kind == QMLE_FOURIER_ANGLE) {
      const double2 cs = trig[l];
      for (int it = threadIdx.x; it < items; it += kFourierThreads) {
        const int node = lv.node_begin + it / F, g = it % F;
        const qmle_fourier_node nd = L.nodes[node];
        const double2 a = child_value(V, nd.cos_child, F, centre, g);
        const double2 sb = times_i_pow(child_value(V, nd.sin_child, F, centre, g), (nd.power + 1) & 3);
        V[(size_t)node * (size_t)F + (size_t)g] = make_double2(cs.x * a.x + cs.y * sb.x, cs.x * a.y + cs.y * sb.y);
      }
    } else {
      const int step = lv.shift * lv.stride;  // flat distance of the shift
      for (int it = threadIdx.x; it < items; it += kFourierThreads) {
        const int node = lv.node_begin + it / F, g = it % F;
        const qmle_fourier_node nd = L.nodes[node];
        const int coord = (g / lv.stride) % lv.dim;
        // (T+ f)(g) = f(g - shift), (T- f)(g) = f(g + shift), zero where the source leaves the axis
        const bool has_p = coord - lv.shift >= 0 && coord - lv.shift < lv.dim;
        const bool has_m = coord + lv.shift >= 0 && coord + lv.shift < lv.dim;
        const double2 zero = make_double2(0.0, 0.0);
        const double2 ap = has_p ? child_value(V, nd.cos_child, F, centre, g - step) : zero;
        const double2 am = has_m ? child_value(V, nd.cos_child, F, centre, g + step) : zero;
        const double2 bp = has_p ? child_value(V, nd.sin_child, F, centre, g - step) : zero;
        const double2 bm = has_m ? child_value(V, nd.sin_child, F, centre, g + step) : zero;
        const double2 sb = times_i_pow(make_double2(bp.x - bm.x, bp.y - bm.y), nd.power & 3);
        V[(size_t)node * (size_t)F + (size_t)g] =
            make_double2(0.5 * ((ap.x + am.x) + sb.x), 0.5 * ((ap.y + am.y) + sb.y));
      }
    }
    __syncthreads();
  }

  double2 *out = L.out + (size_t)b * (size_t)L.n_roots * (size_t)F;
  const int outs = L.n_roots * F;
  for (int it = threadIdx.x; it < outs; it += kFourierThreads) {
    const int r = it / F, g = it % F;
    out[it] = times_i_pow(child_value(V, L.roots[r], F, centre, g), L.roots[L.n_roots + r] & 3);
  }
}

struct FourierLayout {
  size_t nodes, levels, roots, trig, values, total;
};

// false where a size does not fit (the caller answers 0 / QMLE_ERR_INVALID_ARG)
bool fourier_layout(long long n_nodes, long long n_levels, long long n_roots, long long F, long long batch,
                    FourierLayout *lay) {
  if (n_nodes < 0 || n_levels < 0 || n_roots < 1 || F < 1 || batch < 1 || F >= (1ll << 31)) return false;
  if (n_nodes && F > (long long)((size_t)-1 >> 8) / n_nodes / batch) return false;  // 16 batch n_nodes F fits a size_t
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t begin = at;
    at += align_up(bytes, 16);
    return begin;
  };
  lay->nodes = take((size_t)n_nodes * sizeof(qmle_fourier_node));
  lay->levels = take((size_t)n_levels * sizeof(FourierLevel));
  lay->roots = take((size_t)n_roots * 2 * sizeof(int32_t));
  lay->trig = take((size_t)batch * (size_t)n_levels * sizeof(double2));
  lay->values = take((size_t)batch * (size_t)n_nodes * (size_t)F * sizeof(double2));
  lay->total = at < 16 ? 16 : at;
  return true;
}

}  // namespace

extern "C" {

size_t qmle_fourier_workspace_bytes(int n_nodes, int n_levels, int n_roots, int64_t grid_points, int batch) {
  FourierLayout lay;
  return fourier_layout(n_nodes, n_levels, n_roots, grid_points, batch, &lay) ? lay.total : 0;
}

int qmle_fourier_dag(const qmle_fourier_node *nodes, int n_nodes, const qmle_fourier_level *levels, int n_levels,
                     const int32_t *roots, const int32_t *root_phase, int n_roots, const int32_t *dims, int n_axes,
                     const double *d_angles, int n_columns, int batch, void *d_out, void *d_workspace,
                     size_t workspace_bytes, qmle_stream stream_) {
  // every index a lane dereferences is checked here, against the table it points into
  if (n_axes < 0 || n_axes > QMLE_FOURIER_MAX_AXES) return QMLE_ERR_UNSUPPORTED;
  if (batch < 1 || n_roots < 1 || n_nodes < 0 || n_levels < 0 || n_columns < 0 || !roots || !root_phase || !d_out ||
      (n_nodes && !nodes) || (n_levels && !levels) || (n_axes && !dims))
    return QMLE_ERR_INVALID_ARG;
  long long F = 1;
  int32_t stride[QMLE_FOURIER_MAX_AXES + 1];
  for (int a = 0; a < n_axes; ++a) {
    if (dims[a] < 1 || !(dims[a] & 1)) return QMLE_ERR_INVALID_ARG;
    F *= dims[a];
    if (F >= (1ll << 31)) return QMLE_ERR_INVALID_ARG;
  }
  {
    long long s = 1;
    for (int a = n_axes - 1; a >= 0; --a) {
      stride[a] = (int32_t)s;
      s *= dims[a];
    }
  }
  for (int l = 0; l < n_levels; ++l)
    if (levels[l].kind != QMLE_FOURIER_ANGLE && levels[l].kind != QMLE_FOURIER_SHIFT) return QMLE_ERR_UNSUPPORTED;
  std::vector<FourierLevel> dev_levels((size_t)n_levels);
  int expect = 0;
  for (int l = 0; l < n_levels; ++l) {
    const qmle_fourier_level &lv = levels[l];
    if (lv.node_begin != expect || lv.node_end < lv.node_begin || lv.node_end > n_nodes) return QMLE_ERR_INVALID_ARG;
    expect = lv.node_end;
    if ((long long)(lv.node_end - lv.node_begin) * F >= (1ll << 31) - kFourierThreads) return QMLE_ERR_INVALID_ARG;  // `it`
    FourierLevel &d = dev_levels[(size_t)l];
    d = FourierLevel{lv.node_begin, lv.node_end, lv.kind, 0, 0, 1, 1, 0};
    if (lv.kind == QMLE_FOURIER_ANGLE) {
      if (lv.column < 0 || lv.column >= n_columns || !d_angles) return QMLE_ERR_INVALID_ARG;
      d.column = lv.column;
    } else {
      if (lv.axis < 0 || lv.axis >= n_axes) return QMLE_ERR_INVALID_ARG;
      const long long mag = lv.shift < 0 ? -(long long)lv.shift : (long long)lv.shift;
      if (mag == 0 || mag >= dims[lv.axis]) return QMLE_ERR_INVALID_ARG;
      d.shift = lv.shift;
      d.stride = stride[lv.axis];
      d.dim = dims[lv.axis];
    }
    auto child_ok = [&](int32_t c) { return c == QMLE_FOURIER_ONE || c == QMLE_FOURIER_ZERO || (c >= 0 && c < lv.node_begin); };
    for (int j = lv.node_begin; j < lv.node_end; ++j) {
      const qmle_fourier_node &nd = nodes[j];
      if (!child_ok(nd.cos_child) || !child_ok(nd.sin_child) || nd.power < 0 || nd.power > 3)
        return QMLE_ERR_INVALID_ARG;
    }
  }
  if (expect != n_nodes) return QMLE_ERR_INVALID_ARG;
  std::vector<int32_t> dev_roots((size_t)n_roots * 2);
  for (int r = 0; r < n_roots; ++r) {
    const int32_t c = roots[r];
    if (!(c == QMLE_FOURIER_ONE || c == QMLE_FOURIER_ZERO || (c >= 0 && c < n_nodes)) || root_phase[r] < 0 ||
        root_phase[r] > 3)
      return QMLE_ERR_INVALID_ARG;
    dev_roots[(size_t)r] = c;
    dev_roots[(size_t)n_roots + (size_t)r] = root_phase[r];
  }
  if ((long long)n_roots * F >= (1ll << 31) - kFourierThreads) return QMLE_ERR_INVALID_ARG;
  FourierLayout lay;
  if (!fourier_layout(n_nodes, n_levels, n_roots, F, batch, &lay)) return QMLE_ERR_INVALID_ARG;
  if (!d_workspace || workspace_bytes < lay.total || ((uintptr_t)d_workspace & 15u)) return QMLE_ERR_WORKSPACE;

  // the tables travel as asynchronous copies from pageable memory, which the runtime stages before the copy call
  // returns (as the tables of qmle_compose_circuits; the header states what that asks of the caller)
  hipStream_t stream = (hipStream_t)stream_;
  char *base = (char *)d_workspace;
  if (n_nodes)
    HIPCHK(hipMemcpyAsync(base + lay.nodes, nodes, (size_t)n_nodes * sizeof(qmle_fourier_node), hipMemcpyHostToDevice,
                          stream));
  if (n_levels)
    HIPCHK(hipMemcpyAsync(base + lay.levels, dev_levels.data(), dev_levels.size() * sizeof(FourierLevel),
                          hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(base + lay.roots, dev_roots.data(), dev_roots.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                        stream));
  FourierLaunch L{};
  L.nodes = (const qmle_fourier_node *)(base + lay.nodes);
  L.levels = (const FourierLevel *)(base + lay.levels);
  L.roots = (const int32_t *)(base + lay.roots);
  L.angles = d_angles;
  L.trig = (double2 *)(base + lay.trig);
  L.values = (double2 *)(base + lay.values);
  L.out = (double2 *)d_out;
  L.n_nodes = n_nodes;
  L.n_levels = n_levels;
  L.n_roots = n_roots;
  L.n_columns = n_columns;
  L.F = (int32_t)F;
  int32_t centre = 0;
  for (int a = 0; a < n_axes; ++a) centre += (dims[a] - 1) / 2 * stride[a];
  L.centre = centre;
  hipLaunchKernelGGL(k_fourier_dag, dim3((unsigned)batch), dim3(kFourierThreads), 0, stream, L);
  HIPCHK(hipGetLastError());
  return QMLE_OK;
}

}  // extern "C"
