// sdf_lookup.hip -- dgp_sdf_lookup / dgp_sdf_lookup_backward: the reference's bilinear_interpolate (utils/sdf_utils.py:38-107) at arbitrary points of a batch,
// its gradient, and the per-row collision summary behind check_solved (learning/train_initializer.py:81-88) (gfx950 / CDNA4).
//
// What is shared and what is new: pixel coordinates, floor, saturation, clamps and tap offsets are gn_lane.h's obstacle_addr / tiled_tap_offsets / div_res -- the
// lookup of the step, metrics and interpolation kernels, called, not restated (div_res through quot_res below, which keeps the sign of a zero).  New here: the weights, the distance and the Jacobian WITHOUT the hinge
// (obstacle_finish folds eps + radius and the `<=` selection in), and the closed-form gradient.  include/dgpmp2_hip.h states both operation orders,
// tests/lookup_oracle.py restates them, and the kernels are held against that bit for bit.  DGP_TL = 2 (this unit's flag): the grid layout is a run-time branch.
//
// Forward mapping: LPT = 16 / 32 / 64 lanes per batch row, chosen from S (dgp_group::lanes_for), 64 / LPT rows per wavefront.  The lanes of a row walk its points in
// a strided loop, i = lane + k LPT: adjacent lanes read adjacent point rows and store adjacent d_obs / J entries.  A point row moves as ONE vector of two elements
// (8 bytes fp32, 16 bytes fp64) when point_stride == 2 and points / J are aligned to it, element by element otherwise: the access width is the only difference.
// Summary: every lane keeps a count, a first index and a minimum with its index over the fp64 distances of its points, then fixed-order butterflies over the row's
// LPT lanes: no atomics, no LDS, no scratch, the same bits from run to run.  Lanes 0 .. 4 of a row store its DGP_LOOKUP_COUNT doubles as one run.  Lane groups
// past the end of a ragged batch recompute the last row and store nothing (no divergent shuffles).
// Backward mapping: one lane per point in a grid-stride loop; the point's address, taps and weights are recomputed (cheaper than saving 4 weights + 4 offsets per
// point), g_points is one vector / two element stores, the four tap gradients are device-scope atomic adds (gn_device.h's issue: relaxed, agent scope).
// 64-bit indices throughout: B S point_stride may pass 2^31.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#ifndef DGP_TL
#define DGP_TL 2
#endif
#include "dgp_host.h"
#include "dgp_launch.h"
#include "dgp_group.h"

#pragma clang fp contract(off)

namespace {

using dgp_host::fail;

struct LookupArgs {
  dgp::GnParams p;         // the grid and the constants of obstacle_addr: sdf, sdf_rows / cols / bstride / layout, res, inv_res, orig_px, orig_py; B
  const void* points;      // (B, S, >= 2)
  int64_t pstride;         // row pitch in elements
  int32_t S;
  double clearance;
  void* d_obs;             // (B, S) or null
  void* J;                 // (B, S, 2) or null
  double* summary;         // (B, DGP_LOOKUP_COUNT) or null
};
static_assert(sizeof(LookupArgs) <= 4096, "kernel-argument segment");

struct LookupBwdArgs {
  dgp::GnParams p;
  const void* points;
  int64_t pstride;
  int32_t S;
  const void *g_d, *g_J;   // (B, S), (B, S, 2); either may be null (= 0)
  void* g_points;          // (B, S, 2) or null
  void* g_sdf;             // grids in the layout of p.sdf_layout, g_bstride elements apart, or null
  int64_t g_bstride;
  int32_t wide;            // DGP_GSDF_DENSE_F64: g_sdf holds doubles whatever IO is
};
static_assert(sizeof(LookupBwdArgs) <= 4096, "kernel-argument segment");

constexpr int NO_INDEX = 0x7fffffff;
constexpr int kBwdLanes = 256;
constexpr int kBwdMaxBlocks = 1 << 16;           // the rest of the points in the grid-stride loop

// one lookup up to the weights: address (gn_lane.h), the four taps converted to double, the four one-dimensional weights
struct Cell {
  int64_t i11, i21, i12, i22;      // element offsets of dx1y1, dx2y1, dx1y2, dx2y2 inside one grid
  double a, b, c, e;               // their values
  double wja, wjb, wjc, wjd;       // (fy2 - py), (py - fy1), (fx2 - px), (px - fx1)        sdf_utils.py:86-89
};

template <typename IO>
__device__ __forceinline__ void cell_of(const dgp::GnParams& p, const IO* __restrict__ grid, double x, double y, Cell& q) {
  dgp::ObsAddr o;
  dgp::obstacle_addr(p, x, y, o);
  if (dgp::grid_is_tiled(p)) {
    int32_t t11, t21, t12, t22;
    dgp::tiled_tap_offsets(p, o, t11, t21, t12, t22);
    q.i11 = t11; q.i21 = t21; q.i12 = t12; q.i22 = t22;
  } else {
    const int64_t W = p.sdf_cols;
    q.i11 = (int64_t)o.y1 * W + o.x1; q.i21 = (int64_t)o.y1 * W + o.x2; q.i12 = (int64_t)o.y2 * W + o.x1; q.i22 = (int64_t)o.y2 * W + o.x2;
  }
  q.a = (double)grid[q.i11]; q.b = (double)grid[q.i21]; q.c = (double)grid[q.i12]; q.e = (double)grid[q.i22];      // :76-79
  const double fx1 = (double)o.x1, fx2 = (double)o.x2, fy1 = (double)o.y1, fy2 = (double)o.y2;      // the CLAMPED indices against the unclamped px, py (:81-89)
  q.wja = fy2 - o.py; q.wjb = o.py - fy1; q.wjc = fx2 - o.px; q.wjd = o.px - fx1;
}

// u / res as the IEEE quotient: gn_lane.h's div_res, which equals it for every finite non-zero u, with the sign of a zero numerator kept (div_res returns +0 for
// -0: harmless under the hinge of the step kernels; here J and the gradients are held to the reference bit for bit, and a clamped cell gives J = -0.0)
__device__ __forceinline__ double quot_res(const dgp::GnParams& p, double u) { return u == 0.0 ? u : dgp::div_res(p, u); }

// (dgp_rowio.h's rule at D = 2; not its load_row / store_row: through HIP's float2 / double2 both kernels here compile to other code than through these vectors)
template <typename IO, bool VEC>
__device__ __forceinline__ void load_pair(const IO* p, IO& x, IO& y) {
  if (VEC) {
    typedef IO vec_t __attribute__((ext_vector_type(2)));
    const vec_t v = *(const vec_t*)p;
    x = v[0]; y = v[1];
  } else {
    x = p[0]; y = p[1];
  }
}
template <typename IO, bool VEC>
__device__ __forceinline__ void store_pair(IO* p, IO x, IO y) {
  if (VEC) {
    typedef IO vec_t __attribute__((ext_vector_type(2)));
    vec_t v;
    v[0] = x; v[1] = y;
    *(vec_t*)p = v;
  } else {
    p[0] = x; p[1] = y;
  }
}

using dgp_group::group_sum_i;
using dgp_group::group_min_i;

// the minimum with its index: a NaN wins over every number (torch.min), the smaller index wins between equals (and between NaNs).
// Symmetric: both partners of an exchange end with the same pair.  A lane without a point carries (+inf, NO_INDEX) and loses every tie.
template <int LPT>
__device__ __forceinline__ void group_argmin(double& v, int& idx) {
#pragma unroll
  for (int m = 1; m < LPT; m <<= 1) {
    const double ov = __shfl_xor(v, m);
    const int oi = __shfl_xor(idx, m);
    const bool vn = v != v, on = ov != ov;
    const bool less = (on && !vn) || ov < v, equal = (on && vn) || ov == v;
    const bool take = less || (equal && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
  }
}

template <typename IO, int LPT, bool VEC>
__global__ void __launch_bounds__(64) sdf_lookup_kernel(const LookupArgs a) {
  constexpr int TPW = 64 / LPT;
  const dgp::GnParams& p = a.p;
  const int lane = (int)threadIdx.x, l = lane % LPT;
  const int64_t b_raw = (int64_t)blockIdx.x * TPW + lane / LPT;
  const bool on = b_raw < p.B;
  const int64_t b = on ? b_raw : (int64_t)p.B - 1;
  const int S = a.S;
  const IO* pts = (const IO*)a.points + b * S * a.pstride;
  const IO* grid = (const IO*)p.sdf + b * p.sdf_bstride;
  IO* od = (IO*)a.d_obs + b * S;
  IO* oj = (IO*)a.J + b * S * 2;
  const double clr = a.clearance;
  double m_d = __builtin_huge_val();
  int m_idx = NO_INDEX, cnt = 0, first = NO_INDEX;
  for (int i = l; i < S; i += LPT) {
    IO x, y;
    load_pair<IO, VEC>(pts + (int64_t)i * a.pstride, x, y);
    Cell q;
    cell_of<IO>(p, grid, (double)x, (double)y, q);
    const double wa = q.wjc * q.wja;                         // :81-84
    const double wb = q.wjd * q.wja;
    const double wc = q.wjc * q.wjb;
    const double wd = q.wjd * q.wjb;
    const double d = wa * q.a + wb * q.b + wc * q.c + wd * q.e;      // :90, left to right
    if (a.d_obs != nullptr && on) od[i] = (IO)d;
    if (a.J != nullptr) {      // wave-uniform
      const double j0 = quot_res(p, -1.0 * (q.wja * (q.b - q.a) + q.wjb * (q.e - q.c)));      // :93
      const double j1 = quot_res(p, q.wjc * (q.c - q.a) + q.wjd * (q.e - q.b));               // :94
      if (on) store_pair<IO, VEC>(oj + (int64_t)i * 2, (IO)j0, (IO)j1);
    }
    const bool hit = d <= clr;                               // check_solved's comparison: a NaN does not block
    cnt += hit ? 1 : 0;
    first = (hit && i < first) ? i : first;
    const bool take = m_idx == NO_INDEX || (d != d && !(m_d != m_d)) || d < m_d;      // i rises: the smallest index of equals stays
    m_d = take ? d : m_d;
    m_idx = take ? i : m_idx;
  }
  if (a.summary == nullptr) return;
  group_argmin<LPT>(m_d, m_idx);
  cnt = group_sum_i<LPT>(cnt);
  first = group_min_i<LPT>(first);
  double out;
  switch (l) {
    case DGP_LOOKUP_SOLVED: out = cnt > 0 ? 0.0 : 1.0; break;
    case DGP_LOOKUP_NUM_BLOCKED: out = (double)cnt; break;
    case DGP_LOOKUP_FIRST_BLOCKED: out = first == NO_INDEX ? -1.0 : (double)first; break;
    case DGP_LOOKUP_MIN_DIST: out = m_d; break;
    case DGP_LOOKUP_MIN_INDEX: out = (double)m_idx; break;
    default: out = 0.0; break;
  }
  if (on && l < DGP_LOOKUP_COUNT) a.summary[b * DGP_LOOKUP_COUNT + l] = out;
}

template <typename T>
__device__ __forceinline__ void atomic_add(T* p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename IO, bool VEC>
__global__ void __launch_bounds__(kBwdLanes) sdf_lookup_backward_kernel(const LookupBwdArgs a) {
  const dgp::GnParams& p = a.p;
  const int64_t S = a.S, rows = (int64_t)p.B * S, stride = (int64_t)gridDim.x * kBwdLanes;
  const IO *gd_ = (const IO*)a.g_d, *gj_ = (const IO*)a.g_J;
  for (int64_t r = (int64_t)blockIdx.x * kBwdLanes + threadIdx.x; r < rows; r += stride) {
    const int64_t b = r / S;
    IO x, y;
    load_pair<IO, VEC>((const IO*)a.points + r * a.pstride, x, y);
    Cell q;
    cell_of<IO>(p, (const IO*)p.sdf + b * p.sdf_bstride, (double)x, (double)y, q);
    const double gd = gd_ != nullptr ? (double)gd_[r] : 0.0;
    IO j0 = (IO)0, j1 = (IO)0;
    if (gj_ != nullptr) load_pair<IO, VEC>(gj_ + r * 2, j0, j1);
    const double g0 = (double)j0, g1 = (double)j1;
    if (a.g_points != nullptr) {
      // the header's order
      const double cr = quot_res(p, ((q.e - q.c) - q.b) + q.a);
      const double gpx = gd * (q.wja * (q.b - q.a) + q.wjb * (q.e - q.c)) + g1 * cr;
      const double gpy = gd * (q.wjc * (q.c - q.a) + q.wjd * (q.e - q.b)) - g0 * cr;
      store_pair<IO, VEC>((IO*)a.g_points + r * 2, (IO)quot_res(p, gpx), (IO)(-quot_res(p, gpy)));
    }
    if (a.g_sdf != nullptr) {
      const double ta = gd * (q.wjc * q.wja) + quot_res(p, g0 * q.wja - g1 * q.wjc);
      const double tb = gd * (q.wjd * q.wja) - quot_res(p, g0 * q.wja + g1 * q.wjd);
      const double tc = gd * (q.wjc * q.wjb) + quot_res(p, g0 * q.wjb + g1 * q.wjc);
      const double te = gd * (q.wjd * q.wjb) + quot_res(p, g1 * q.wjd - g0 * q.wjb);
      const int64_t g0_ = b * a.g_bstride;
      if (sizeof(IO) == 8 || a.wide) {      // fp64 accumulators: the contribution unrounded
        double* g = (double*)a.g_sdf + g0_;
        atomic_add(g + q.i11, ta); atomic_add(g + q.i21, tb); atomic_add(g + q.i12, tc); atomic_add(g + q.i22, te);
      } else {                              // accumulators of the I/O type: rounded once, then added
        float* g = (float*)a.g_sdf + g0_;
        atomic_add(g + q.i11, (float)ta); atomic_add(g + q.i21, (float)tb); atomic_add(g + q.i12, (float)tc); atomic_add(g + q.i22, (float)te);
      }
    }
  }
}

bool aligned(const void* p, size_t bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }      // (null counts as aligned)

template <typename IO, bool VEC>
hipError_t launch_fwd(int lpt, const LookupArgs& a, hipStream_t s, const dgp_dev::Events& ev) {
  const int tpw = 64 / lpt;
  const dim3 grid((unsigned)(((int64_t)a.p.B + tpw - 1) / tpw)), block(64);
  return dgp_dev::with_lpt(lpt, [&](auto L) { return dgp_dev::launch(sdf_lookup_kernel<IO, L, VEC>, grid, block, 0, s, ev, a); });
}

template <typename IO>
hipError_t launch_fwd_io(const LookupArgs& a, hipStream_t s, const dgp_dev::Events& ev) {
  const bool vec = a.pstride == 2 && aligned(a.points, 2 * sizeof(IO)) && aligned(a.J, 2 * sizeof(IO));
  const int lpt = dgp_group::lanes_for(a.S);
  return vec ? launch_fwd<IO, true>(lpt, a, s, ev) : launch_fwd<IO, false>(lpt, a, s, ev);
}

template <typename IO>
hipError_t launch_bwd_io(const LookupBwdArgs& a, hipStream_t s, const dgp_dev::Events& ev) {
  const bool vec = a.pstride == 2 && aligned(a.points, 2 * sizeof(IO)) && aligned(a.g_J, 2 * sizeof(IO)) && aligned(a.g_points, 2 * sizeof(IO));
  const int64_t rows = (int64_t)a.p.B * a.S, want = (rows + kBwdLanes - 1) / kBwdLanes;
  const dim3 grid((unsigned)(want < kBwdMaxBlocks ? want : kBwdMaxBlocks)), block(kBwdLanes);
  if (vec) return dgp_dev::launch(sdf_lookup_backward_kernel<IO, true>, grid, block, 0, s, ev, a);
  return dgp_dev::launch(sdf_lookup_backward_kernel<IO, false>, grid, block, 0, s, ev, a);
}

// the checks both entry points share, and the constants of obstacle_addr formed as dgp_host::fill_call forms them
int fill_common(const char* who, int32_t dtype, int32_t batch, int32_t num_points, const void* points, int64_t point_stride, const DgpSdf* sdf, double res,
                const double* x_lims, const double* y_lims, dgp::GnParams& p) {
  if (dtype != DGP_F32 && dtype != DGP_F64) return fail(DGP_EINVAL, "%s: dtype must be DGP_F32 or DGP_F64, got %d", who, dtype);
  if (batch < 1 || num_points < 1) return fail(DGP_EINVAL, "%s: batch and num_points must be positive, got %d and %d", who, batch, num_points);
  if (!points) return fail(DGP_EINVAL, "%s: null points", who);
  if (point_stride < 2) return fail(DGP_EINVAL, "%s: point_stride must be >= 2 (x and y are the first two elements of a row), got %lld", who, (long long)point_stride);
  if (!sdf || !sdf->data) return fail(DGP_EINVAL, "%s: sdf must be non-null", who);
  if (sdf->rows < 1 || sdf->cols < 1) return fail(DGP_EINVAL, "%s: sdf grid must be at least 1x1, got %dx%d", who, sdf->rows, sdf->cols);
  if (sdf->cols < 2) return fail(DGP_EUNSUPPORTED, "%s: sdf grids with a single column are not implemented", who);
  if (sdf->batch_stride < 0) return fail(DGP_EINVAL, "%s: negative sdf batch stride", who);
  if (((int64_t)sdf->rows + 3) * ((int64_t)sdf->cols + 3) >= ((int64_t)1 << 31)) return fail(DGP_EUNSUPPORTED, "%s: sdf grid of %dx%d elements is too large", who, sdf->rows, sdf->cols);
  if (sdf->layout != DGP_SDF_ROWMAJOR && sdf->layout != DGP_SDF_TILED4) return fail(DGP_EINVAL, "%s: bad DgpSdf::layout %d", who, sdf->layout);
  if (!(res > 0.0) || !(res <= DBL_MAX)) return fail(DGP_EINVAL, "%s: res must be positive and finite", who);
  if (!x_lims || !y_lims) return fail(DGP_EINVAL, "%s: null x_lims or y_lims", who);
  if (!(x_lims[1] > x_lims[0]) || !(y_lims[1] > y_lims[0])) return fail(DGP_EINVAL, "%s: empty or reversed x/y limits", who);
  memset(&p, 0, sizeof(p));
  p.B = batch;
  p.sdf = sdf->data; p.sdf_rows = sdf->rows; p.sdf_cols = sdf->cols; p.sdf_bstride = sdf->batch_stride; p.sdf_layout = sdf->layout;
  p.res = res;
  p.inv_res = 1.0 / p.res;
  p.orig_px = (0. - x_lims[0] / p.res);      // sdf_utils.py:57-58
  p.orig_py = (0. - y_lims[0] / p.res);
  return DGP_OK;
}

}  // namespace

extern "C" int dgp_sdf_lookup(int32_t dtype, int32_t batch, int32_t num_points, const void* points, int64_t point_stride, const DgpSdf* sdf, double res,
                              const double* x_lims, const double* y_lims, double clearance, void* d_obs, void* J, double* summary, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  LookupArgs a;
  const int rc = fill_common("dgp_sdf_lookup", dtype, batch, num_points, points, point_stride, sdf, res, x_lims, y_lims, a.p);
  if (rc != DGP_OK) return rc;
  if (!d_obs && !J && !summary) return fail(DGP_EINVAL, "dgp_sdf_lookup: d_obs, J and summary are all null");
  if (summary && !(clearance >= -DBL_MAX && clearance <= DBL_MAX)) return fail(DGP_EINVAL, "dgp_sdf_lookup: the summary needs a finite clearance");
  a.points = points; a.pstride = point_stride; a.S = num_points; a.clearance = clearance;
  a.d_obs = d_obs; a.J = J; a.summary = summary;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = dtype == DGP_F64 ? launch_fwd_io<double>(a, s, ev) : launch_fwd_io<float>(a, s, ev);
  return dgp_dev::hip_rc(e, "dgp_sdf_lookup");
}

extern "C" int dgp_sdf_lookup_backward(int32_t dtype, int32_t batch, int32_t num_points, const void* points, int64_t point_stride, const DgpSdf* sdf, double res,
                                       const double* x_lims, const double* y_lims, const void* g_d, const void* g_J, void* g_points, void* g_sdf,
                                       int64_t g_sdf_batch_stride, int32_t g_sdf_copies, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  LookupBwdArgs a;
  const int rc = fill_common("dgp_sdf_lookup_backward", dtype, batch, num_points, points, point_stride, sdf, res, x_lims, y_lims, a.p);
  if (rc != DGP_OK) return rc;
  if (!g_d && !g_J) return fail(DGP_EINVAL, "dgp_sdf_lookup_backward: g_d and g_J are both null (no cotangent)");
  if (!g_points && !g_sdf) return fail(DGP_EINVAL, "dgp_sdf_lookup_backward: g_points and g_sdf are both null");
  if (g_sdf_batch_stride < 0) return fail(DGP_EINVAL, "dgp_sdf_lookup_backward: negative g_sdf batch stride");
  if (g_sdf_copies < 1) return fail(DGP_EINVAL, "dgp_sdf_lookup_backward: g_sdf_copies must be 1, got %d", g_sdf_copies);
  if (g_sdf_copies != 1) return fail(DGP_EUNSUPPORTED, "dgp_sdf_lookup_backward: partial copies of the grid gradient are not implemented (g_sdf_copies must be 1)");
  if (sdf->grad_mode == DGP_GSDF_SPARSE) return fail(DGP_EUNSUPPORTED, "dgp_sdf_lookup_backward: DGP_GSDF_SPARSE is not implemented (DGP_GSDF_DENSE or DGP_GSDF_DENSE_F64)");
  if (sdf->grad_mode != DGP_GSDF_DENSE && sdf->grad_mode != DGP_GSDF_DENSE_F64) return fail(DGP_EINVAL, "dgp_sdf_lookup_backward: bad DgpSdf::grad_mode %d", sdf->grad_mode);
  a.points = points; a.pstride = point_stride; a.S = num_points; a.g_d = g_d; a.g_J = g_J;
  a.g_points = g_points; a.g_sdf = g_sdf; a.g_bstride = g_sdf_batch_stride; a.wide = sdf->grad_mode == DGP_GSDF_DENSE_F64 ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = dtype == DGP_F64 ? launch_bwd_io<double>(a, s, ev) : launch_bwd_io<float>(a, s, ev);
  return dgp_dev::hip_rc(e, "dgp_sdf_lookup_backward");
}
