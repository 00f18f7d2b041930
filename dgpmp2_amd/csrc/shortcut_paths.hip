// shortcut_paths.hip -- dgp_shortcut_paths: line-of-sight shortcutting of the grid paths of dgp_init_paths, ONE launch (gfx950 / CDNA4).
//
// What it stands in for: the simplifySolution() call RRTStar.plan makes before interpolate(num_states) (diff_gpmp2/ompl_rrtstar.py:36-41): the trajectory the
// reference's Gauss-Newton receives is a short any-angle polyline, not a tree path.  Here: one greedy pass of string pulling over the vertices start -> traced
// cells -> goal, a segment being usable where every point of OMPL's discrete motion check is feasible by Env2D.is_feasible -- the sampler's bilinear distance
// (csrc/problem_sampler.hip, restated below for row-major grids: the same pixel coordinates, clamps, weights and operation order -- lifted into one function the
// distance leaves shortcut_paths_kernel as it is but recompiles sample_problems_kernel<double> to code measured 0.5 % slower) above the clearance.
// include/dgpmp2_hip.h states the rule, tests/shortcut_oracle.py restates it, and the kernel is held against that bit for bit.
//
// Mapping: one wavefront (one workgroup of 64) per problem, as init_paths.hip.  The hot path is visible(P, Q): the M + 1 check points of a segment go over the 64
// lanes, T = ceil((M + 1) / 64) trips, lane l taking the points l T + t in trip t -- every trip samples the whole segment at a spacing of T points, so a blocked
// segment nearly always fails in its first trip (visible is a pure predicate: the order its points are tested in decides nothing).  Each lane does the four-tap
// lookup of its point; one ballot of the infeasible lanes ends the segment.  The candidates j of an anchor are tested from the far end down, one after the other:
// the first visible one is the largest.  Control flow is wave-uniform throughout (anchor, candidate, M and the ballot are the same in every lane); only the tap
// addresses differ per lane.  (Packing 64 short candidates into one trip was not built: near the anchor a candidate has few points, but it is reached only after
// every farther one has failed, and those dominate.)
// The kept set is one bit per traced cell in dynamic LDS (path_cap bits; V_0 and V_{L+1} are always kept); the second pass walks the set bits and lane l places
// rows l, l + 64, ... as the segment they fall in comes by, exactly as the second walk of init_paths.hip.
// The traced cells are read as numbers only (a cell index never addresses memory), and every tap is clamped: no input value can take a load out of its grid.
// Every loop is bounded by L, lookahead or M (<= 2^20).  No atomics, nothing allocated or synchronised.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dgp_status.h"
#include "dgp_launch.h"

#pragma clang fp contract(off)

namespace {

using dgp_host::fail;

constexpr int MAX_SIDE = 1 << 12;
constexpr int MAX_PATH_CAP = 1 << 18;
constexpr double MAX_M = 1048576.0;      // 2^20 check intervals; a segment that would need more is not visible

struct ShortcutArgs {
  const void* sdf;
  int64_t sdf_bstride;
  int32_t H, W, B, n;
  const int32_t* env_index;      // (B) or null
  const void *start, *goal;
  const int32_t *path_cells, *num_cells;
  void* th;
  int32_t *vertex_index, *num_vertices, *info;      // each may be null
  double* length;                                   // may be null
  double clearance, check_step, res, inv_res, orig_x, orig_y, total_time_sec;
  double max_d, xlo, xhi, ylo, yhi;
  int32_t path_cap, vertex_cap, lookahead;
};

// a / res as the IEEE quotient (gn_lane.h's div_res, the sampler's: one exact-residual correction on a * (1 / res), 1 / res correctly rounded on the host)
__device__ __forceinline__ double div_res(const ShortcutArgs& a, double v) {
  const double q0 = v * a.inv_res;
  const double r = __builtin_fma(-q0, a.res, v);
  return __builtin_fma(r, a.inv_res, q0);
}

// Env2D.is_feasible (env_2d.py:86-90, :119-175): signed_distance of csrc/problem_sampler.hip for a row-major grid, then `> clearance`
template <typename IO>
__device__ __forceinline__ bool feasible(const ShortcutArgs& a, const IO* __restrict__ grid, double x, double y) {
  const double px = a.orig_x + div_res(a, x), py = a.orig_y - div_res(a, y);
  const double big = 1.0e9;      // (saturate before the conversion; fmax / fmin return the non-NaN operand)
  const double cx = fmin(fmax(floor(px), -big), big), cy = fmin(fmax(floor(py), -big), big);
  const int32_t x1r = (int32_t)cx, y1r = (int32_t)cy;
  const int32_t W1 = a.W - 1, H1 = a.H - 1;
  const int32_t x1 = max(0, min(x1r, W1)), x2 = max(0, min(x1r + 1, W1)), y1 = max(0, min(y1r, H1)), y2 = max(0, min(y1r + 1, H1));
  const double d11 = (double)grid[y1 * a.W + x1], d21 = (double)grid[y1 * a.W + x2], d12 = (double)grid[y2 * a.W + x1], d22 = (double)grid[y2 * a.W + x2];
  const double fx1 = (double)x1, fx2 = (double)x2, fy1 = (double)y1, fy2 = (double)y2;      // the CLAMPED indices (:144-147)
  const double wa = (fx2 - px) * (fy2 - py);
  const double wb = (px - fx1) * (fy2 - py);
  const double wc = (fx2 - px) * (py - fy1);
  const double wd = (px - fx1) * (py - fy1);
  const double dist = wa * d11 + wb * d21 + wc * d12 + wd * d22;      // :153
  const bool inlim = x <= a.xhi && x >= a.xlo && y <= a.yhi && y >= a.ylo;      // closed on both sides; NaN: outside
  return (inlim ? dist : a.max_d) > a.clearance;
}

// visible(P, Q): wave-uniform arguments, wave-uniform result
template <typename IO>
__device__ __forceinline__ bool visible(const ShortcutArgs& a, const IO* __restrict__ grid, double px, double py, double qx, double qy, int lane) {
  const double dx = qx - px, dy = qy - py;
  const double m = fmax(fabs(dx), fabs(dy)) / a.check_step;
  if (m > MAX_M) return false;
  const int M = !(m > 1.0) ? 1 : (int)ceil(m);
  const double Md = (double)M;
  const int T = (M + 64) >> 6;      // ceil((M + 1) / 64)
  for (int t = 0; t < T; ++t) {
    const int k = lane * T + t;
    bool bad = false;
    if (k <= M) {
      const double f = (double)k / Md;
      bad = !feasible<IO>(a, grid, px + f * dx, py + f * dy);
    }
    if (__ballot(bad) != 0ull) return false;
  }
  return true;
}

template <typename IO>
__global__ void __launch_bounds__(64) shortcut_paths_kernel(const ShortcutArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_keep[];      // bit j - 1: vertex j (1 .. L) is kept
  const int lane = (int)threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x;
  const int n = a.n, N = n - 1;
  const int64_t env = a.env_index != nullptr ? (int64_t)a.env_index[b] : b;
  const IO* __restrict__ grid = (const IO*)a.sdf + env * a.sdf_bstride;
  const IO* so = (const IO*)a.start + b * 4;
  const IO* go = (const IO*)a.goal + b * 4;
  const double sx = (double)so[0], sy = (double)so[1], gx = (double)go[0], gy = (double)go[1];
  const int32_t* cells = a.path_cells + b * (int64_t)a.path_cap;
  const int L = __builtin_amdgcn_readfirstlane(a.num_cells[b]);
  int32_t* vidx = a.vertex_index != nullptr ? a.vertex_index + b * (int64_t)a.vertex_cap : nullptr;

  int flags = (L <= 0 ? 1 : 0) | (L > a.path_cap ? 2 : 0);
  if (flags != 0) {      // nothing to simplify: th stays as it is
    if (vidx != nullptr)
      for (int k = lane; k < a.vertex_cap; k += 64) vidx[k] = -1;
    if (lane == 0) {
      if (a.num_vertices != nullptr) a.num_vertices[b] = 0;
      if (a.length != nullptr) a.length[b] = -1.0;
      if (a.info != nullptr) a.info[b] = flags;
    }
    return;
  }

  const int W = a.W;
  auto vertex = [&](int j, double& x, double& y) {      // V_j, 0 .. L + 1
    if (j == 0) { x = sx; y = sy; }
    else if (j == L + 1) { x = gx; y = gy; }
    else {
      const int cell = __builtin_amdgcn_readfirstlane(cells[j - 1]);
      const int r = cell / W, c = cell % W;
      x = ((double)c - a.orig_x) * a.res; y = (a.orig_y - (double)r) * a.res;
    }
  };

  const int words = (L + 31) >> 5;
  for (int w = lane; w < words; w += 64) s_keep[w] = 0u;
  __syncthreads();

  // first pass: the greedy search -> the kept set, m, S
  int kept = 1, at = 0;
  double px = sx, py = sy, S = 0.0;
  if (vidx != nullptr && lane == 0 && a.vertex_cap > 0) vidx[0] = 0;
  while (at < L + 1) {
    const int hi = min(L + 1, at + a.lookahead);
    int jstar = at + 1;
    double qx = 0.0, qy = 0.0;
    for (int j = hi; j >= at + 2; --j) {
      vertex(j, qx, qy);
      if (visible<IO>(a, grid, px, py, qx, qy, lane)) { jstar = j; break; }
    }
    if (jstar == at + 1) {      // kept whether or not it is visible
      vertex(jstar, qx, qy);
      if (!visible<IO>(a, grid, px, py, qx, qy, lane)) flags |= 8;
    }
    const double dx = qx - px, dy = qy - py;
    S = S + sqrt(dx * dx + dy * dy);
    if (lane == 0) {
      if (jstar <= L) s_keep[(jstar - 1) >> 5] |= 1u << ((jstar - 1) & 31);
      if (vidx != nullptr && kept < a.vertex_cap) vidx[kept] = jstar;
    }
    ++kept;
    at = jstar; px = qx; py = qy;
  }
  if (kept > a.vertex_cap) flags |= 4;
  __syncthreads();

  // second pass: lane l places rows l, l + 64, ... < N; row i lies on segment j, the lowest j with s_{j+1} >= t_i = S i / N
  IO* th = (IO*)a.th + b * (int64_t)n * 4;
  const double vx = (gx - sx) / a.total_time_sec, vy = (gy - sy) / a.total_time_sec;
  const double Nd = (double)N;
  int i = lane;
  double s = 0.0;
  px = sx; py = sy;
  auto segment = [&](double x, double y) {
    const double dx = x - px, dy = y - py;
    const double len = sqrt(dx * dx + dy * dy), s1 = s + len;
    while (i < N) {
      const double t = S * (double)i / Nd;
      if (!(t <= s1)) break;
      const double f = len > 0.0 ? (t - s) / len : 0.0;
      th[i * 4] = (IO)(px + f * dx); th[i * 4 + 1] = (IO)(py + f * dy); th[i * 4 + 2] = (IO)vx; th[i * 4 + 3] = (IO)vy;
      i += 64;
    }
    return s1;
  };
  for (int w = 0; w < words; ++w) {
    uint32_t bits = s_keep[w];      // (one address for the wave: a broadcast)
    while (bits != 0u) {
      const int j = w * 32 + __builtin_ctz(bits) + 1;
      bits &= bits - 1u;
      double x, y;
      vertex(j, x, y);
      s = segment(x, y);
      px = x; py = y;
    }
  }
  {
    const double dx = gx - px, dy = gy - py;
    const double len = sqrt(dx * dx + dy * dy);
    segment(gx, gy);
    for (; i < N; i += 64) {      // (t_i beyond the last arc length: the last segment)
      const double t = S * (double)i / Nd;
      const double f = len > 0.0 ? (t - s) / len : 0.0;
      th[i * 4] = (IO)(px + f * dx); th[i * 4 + 1] = (IO)(py + f * dy); th[i * 4 + 2] = (IO)vx; th[i * 4 + 3] = (IO)vy;
    }
  }
  if (lane == 0) { th[N * 4] = (IO)gx; th[N * 4 + 1] = (IO)gy; th[N * 4 + 2] = (IO)vx; th[N * 4 + 3] = (IO)vy; }      // row N: the goal point itself
  if (vidx != nullptr)
    for (int k = min(kept, a.vertex_cap) + lane; k < a.vertex_cap; k += 64) vidx[k] = -1;
  if (lane == 0) {
    if (a.num_vertices != nullptr) a.num_vertices[b] = kept;
    if (a.length != nullptr) a.length[b] = S;
    if (a.info != nullptr) a.info[b] = flags;
  }
}

}  // namespace

extern "C" int dgp_shortcut_paths(const DgpHandle* h, int32_t batch, const DgpSdf* sdf, const int32_t* env_index, const DgpShortcutParams* p, const void* start,
                                  const void* goal, const int32_t* path_cells, const int32_t* num_cells, void* th, int32_t* vertex_index, int32_t* num_vertices,
                                  double* length, int32_t* info, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  dgp_dev::RowMajorGrid g;
  const int rc = dgp_dev::rowmajor_grid("dgp_shortcut_paths", h, batch, sdf, p, "DgpShortcutParams", start && goal && path_cells && num_cells && th,
                                        "start, goal, path_cells, num_cells and th", MAX_SIDE, g);
  if (rc != DGP_OK) return rc;
  const DgpConfig& c = *g.cfg;
  if (!(p->clearance == p->clearance)) return fail(DGP_EINVAL, "dgp_shortcut_paths: NaN clearance");
  const double res = g.res;
  if (!(p->check_step - p->check_step == 0.0) || !(p->check_step >= res / 16.0))
    return fail(DGP_EINVAL, "dgp_shortcut_paths: check_step must be finite and >= res / 16 = %g, got %g", res / 16.0, p->check_step);
  if (p->path_cap < 1 || p->path_cap > MAX_PATH_CAP) return fail(DGP_EINVAL, "dgp_shortcut_paths: path_cap must be in 1..%d, got %d", MAX_PATH_CAP, p->path_cap);
  if (p->vertex_cap < 0) return fail(DGP_EINVAL, "dgp_shortcut_paths: vertex_cap must be >= 0, got %d", p->vertex_cap);
  if (p->lookahead < 1) return fail(DGP_EINVAL, "dgp_shortcut_paths: lookahead must be >= 1, got %d", p->lookahead);
  if (vertex_index && p->vertex_cap == 0) return fail(DGP_EINVAL, "dgp_shortcut_paths: vertex_index needs vertex_cap >= 1");
  ShortcutArgs a;
  a.sdf = sdf->data; a.sdf_bstride = sdf->batch_stride; a.H = sdf->rows; a.W = sdf->cols; a.B = batch; a.n = c.num_states;
  a.env_index = env_index; a.start = start; a.goal = goal; a.path_cells = path_cells; a.num_cells = num_cells; a.th = th;
  a.vertex_index = vertex_index; a.num_vertices = num_vertices; a.info = info; a.length = length;
  a.clearance = p->clearance; a.check_step = p->check_step;
  a.res = res; a.inv_res = 1.0 / res; a.orig_x = g.orig_x; a.orig_y = g.orig_y;
  a.total_time_sec = c.total_time_sec;
  a.max_d = c.x_lims[1] - c.x_lims[0];      // Env2D.MAX_D: the distance of a point outside the limits
  a.xlo = c.x_lims[0]; a.xhi = c.x_lims[1]; a.ylo = c.y_lims[0]; a.yhi = c.y_lims[1];
  a.path_cap = p->path_cap; a.vertex_cap = p->vertex_cap; a.lookahead = p->lookahead > (1 << 30) ? (1 << 30) : p->lookahead;      // (at + lookahead stays inside int32)
  const dim3 grid((unsigned)batch), block(64);
  const unsigned lds = (((unsigned)a.path_cap + 127u) >> 7) * 16u;      // path_cap bits, in whole 16-byte slots
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = c.io_dtype == DGP_F64 ? dgp_dev::launch(shortcut_paths_kernel<double>, grid, block, lds, s, ev, a)
                                             : dgp_dev::launch(shortcut_paths_kernel<float>, grid, block, lds, s, ev, a);
  return dgp_dev::hip_rc(e, "dgp_shortcut_paths");
}
