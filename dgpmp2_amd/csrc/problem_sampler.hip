// problem_sampler.hip -- dgp_sample_problems: feasible start / goal pairs and their straight-line initial trajectories for a batch of planning problems in ONE launch
// (gfx950 / CDNA4).
//
// What it replaces: the rejection loops of the reference's dataset generation, one Env2D.is_feasible call (a dozen small torch kernels) per candidate point --
// get_random_2d_confs / generate_start_goal (datasets/generate_optimal_paths_gpmp2.py:54-81, :120-162) over Env2D.is_feasible / get_signed_obstacle_distance
// (env/env_2d.py:86-90, :119-175), and straight_line_trajb (utils/planner_utils.py:47-56).  include/dgpmp2_hip.h states the rule.
//
// Randomness: Philox4x32-10, key = the seed, counter = (problem lo, problem hi, draw index k, stream); one block of four words is one candidate point.  Candidate k
// of a problem is a pure function of (seed, problem number, k): the sequential rule "the lowest k that is accepted" needs no sequential loop.
// Mapping: GW = 16 lanes per problem, 4 problems per wavefront.  Per round the 16 lanes of a problem evaluate candidates k0 .. k0 + 15 (16 dependent, divergent tap
// fetches in flight per problem instead of one), a ballot gives the first accepted lane, and the near-tries rule of the goal loop -- "accepted once more than
// near_tries feasible-but-near candidates came before" -- is the prefix population count of the round's feasible-but-near mask on top of the count carried over from
// the rounds before: exactly the sequential result, whatever the batch size, the position in the batch or the grid layout.  Why 16: the reference's environments
// accept a candidate with probability 0.3 .. 0.9, so one round nearly always ends a loop (a wider group would only draw candidates nobody needs), and 16 lanes store
// 64 / 128 contiguous bytes of th_init per instruction.  The ballots and shuffles run in wave-uniform control flow (the loops test __any): only the tap fetches sit
// behind a per-lane branch.  Lane groups past the end of a ragged batch recompute the last problem and store nothing.
// The lookup: gn_lane.h's obstacle_addr and tiled_tap_offsets -- the pixel coordinates, floor, clamps and tap offsets of the step and metrics kernels, both layouts
// (DGP_TL = 2, this unit's flag: a run-time branch) -- and the distance in the reference's operation order, contraction off; no hinge here: a point is feasible where
// dist > clearance.  No atomics, nothing allocated or synchronised.
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifndef DGP_TL
#define DGP_TL 2
#endif
#include "dgp_host.h"
#include "dgp_launch.h"
#include "dgp_philox.h"

namespace {

using dgp_host::fail;
using dgp::philox4x32_10;

constexpr int GW = 16;      // lanes per problem

struct SampleArgs {
  dgp::GnParams p;          // B, n, the grid and the constants of the lookup (dgp_host::fill_call)
  const int32_t* env_index; // (B) or null
  const int32_t* diagonal;  // (B) or null
  void *start, *goal, *th_init;
  int32_t* draws;           // (B, 2) or null
  int32_t* info;            // (B) or null
  uint64_t first_problem;
  uint32_t key0, key1;
  int32_t near_tries, max_draws;
  double clearance;
  double lbx, lby, wx, wy;  // sampling box: lower corner and extent
  double min_dist;          // min_dist_frac * the box diagonal
  double max_d;             // Env2D.MAX_D = x_max - x_min: the distance of a point outside the limits
  double xlo, xhi, ylo, yhi;
  double cxlo, cxhi, cylo, cyhi;      // the corners of the diagonal problems: the limits moved in by corner_inset
  double total_time_sec;
};
static_assert(sizeof(SampleArgs) <= 4096, "kernel-argument segment");

// candidate k of `problem` in stream 0 (start) / 1 (goal)
__device__ __forceinline__ void candidate(const SampleArgs& a, uint64_t problem, uint32_t k, uint32_t stream, double& x, double& y) {
#pragma clang fp contract(off)
  uint32_t w[4];
  philox4x32_10((uint32_t)problem, (uint32_t)(problem >> 32), k, stream, a.key0, a.key1, w);
  const double u0 = (double)((((uint64_t)w[0] << 32) | w[1]) >> 11) * 0x1.0p-53;
  const double u1 = (double)((((uint64_t)w[2] << 32) | w[3]) >> 11) * 0x1.0p-53;
  x = a.lbx + u0 * a.wx;
  y = a.lby + u1 * a.wy;
}

// Env2D.get_signed_obstacle_distance (env_2d.py:119-175) of one point, fp64, the reference's operation order
template <typename IO>
__device__ __forceinline__ double signed_distance(const SampleArgs& a, const IO* __restrict__ grid, double x, double y) {
#pragma clang fp contract(off)
  const dgp::GnParams& p = a.p;
  dgp::ObsAddr o;
  dgp::obstacle_addr(p, x, y, o);
  int64_t i11, i21, i12, i22;
  if (dgp::grid_is_tiled(p)) {
    int32_t t11, t21, t12, t22;
    dgp::tiled_tap_offsets(p, o, t11, t21, t12, t22);
    i11 = t11; i21 = t21; i12 = t12; i22 = t22;
  } else {
    const int64_t W = p.sdf_cols;
    i11 = (int64_t)o.y1 * W + o.x1; i21 = (int64_t)o.y1 * W + o.x2; i12 = (int64_t)o.y2 * W + o.x1; i22 = (int64_t)o.y2 * W + o.x2;
  }
  const double d11 = (double)grid[i11], d21 = (double)grid[i21], d12 = (double)grid[i12], d22 = (double)grid[i22];      // :139-142
  const double fx1 = (double)o.x1, fx2 = (double)o.x2, fy1 = (double)o.y1, fy2 = (double)o.y2;      // the CLAMPED indices, as the reference has them at :144-147
  const double wa = (fx2 - o.px) * (fy2 - o.py);
  const double wb = (o.px - fx1) * (fy2 - o.py);
  const double wc = (fx2 - o.px) * (o.py - fy1);
  const double wd = (o.px - fx1) * (o.py - fy1);
  const double dist = wa * d11 + wb * d21 + wc * d12 + wd * d22;      // :153
  const bool inlim = x <= a.xhi && x >= a.xlo && y <= a.yhi && y >= a.ylo;      // :159-166 (closed on both sides; NaN: outside)
  return inlim ? dist : a.max_d;      // :169
}

__device__ __forceinline__ uint32_t group_mask(bool pred, int shift) { return (uint32_t)(__ballot(pred) >> shift) & ((1u << GW) - 1u); }

template <typename IO>
__global__ void __launch_bounds__(64) sample_problems_kernel(const SampleArgs a) {
#pragma clang fp contract(off)
  constexpr int PPW = 64 / GW;
  const dgp::GnParams& p = a.p;
  const int lane = (int)threadIdx.x, l = lane % GW, gbase = lane - l;
  const int64_t b_raw = (int64_t)blockIdx.x * PPW + lane / GW;
  const bool on = b_raw < p.B;
  const int64_t b = on ? b_raw : (int64_t)p.B - 1;
  const uint64_t problem = a.first_problem + (uint64_t)b;
  const int64_t env = a.env_index != nullptr ? (int64_t)a.env_index[b] : b;
  const IO* grid = (const IO*)p.sdf + env * p.sdf_bstride;
  const int diag = a.diagonal != nullptr ? a.diagonal[b] : -1;
  const int max_draws = a.max_draws;

  double sx = 0.0, sy = 0.0, gx = 0.0, gy = 0.0;
  int draw_s = -1, draw_g = -1, flags = 0;
  bool random = true;
  if (diag >= 0 && diag <= 3) {      // generate_optimal_paths_gpmp2.py:134-148: corner to corner, unless a corner is infeasible
    const bool s_hi_x = diag == 1 || diag == 2, s_hi_y = diag == 1 || diag == 3;
    sx = s_hi_x ? a.cxhi : a.cxlo; sy = s_hi_y ? a.cyhi : a.cylo;
    gx = s_hi_x ? a.cxlo : a.cxhi; gy = s_hi_y ? a.cylo : a.cyhi;
    random = !(signed_distance<IO>(a, grid, sx, sy) > a.clearance && signed_distance<IO>(a, grid, gx, gy) > a.clearance);
    if (random) flags |= 8;
  }

  // start loop (:63-67): the lowest k whose candidate is feasible
  bool act = random;
  int k0 = 0;
  while (__any(act)) {
    const int k = k0 + l;
    const bool in = act && k < max_draws;
    double cx = 0.0, cy = 0.0;
    bool feas = false;
    if (in) {
      candidate(a, problem, (uint32_t)k, 0u, cx, cy);
      feas = signed_distance<IO>(a, grid, cx, cy) > a.clearance;
    }
    const uint32_t fm = group_mask(feas, gbase);
    const bool last = max_draws - k0 <= GW;
    const int src = fm != 0u ? __builtin_ctz(fm) : (max_draws - 1 - k0) & (GW - 1);      // no acceptance in the last round: the last candidate drawn
    const double bx = __shfl(cx, gbase + src), by = __shfl(cy, gbase + src);
    if (act && (fm != 0u || last)) {
      sx = bx; sy = by; draw_s = k0 + src;
      if (fm == 0u) flags |= 1;
      act = false;
    }
    k0 += GW;
  }

  // goal loop (:69-80): the lowest k whose candidate is feasible and either far enough from the start or preceded by more than near_tries feasible-but-near ones
  act = random;
  k0 = 0;
  int tries = 0;
  while (__any(act)) {
    const int k = k0 + l;
    const bool in = act && k < max_draws;
    double cx = 0.0, cy = 0.0;
    bool feas = false, far = false;
    if (in) {
      candidate(a, problem, (uint32_t)k, 1u, cx, cy);
      feas = signed_distance<IO>(a, grid, cx, cy) > a.clearance;
      const double dx = cx - sx, dy = cy - sy;
      far = sqrt(dx * dx + dy * dy) >= a.min_dist;
    }
    const uint32_t nm = group_mask(feas && !far, gbase);
    const int before = tries + __popc(nm & ((1u << l) - 1u));
    const uint32_t am = group_mask(feas && (far || before > a.near_tries), gbase);
    const bool last = max_draws - k0 <= GW;
    const int src = am != 0u ? __builtin_ctz(am) : (max_draws - 1 - k0) & (GW - 1);
    const double bx = __shfl(cx, gbase + src), by = __shfl(cy, gbase + src);
    if (act && (am != 0u || last)) {
      gx = bx; gy = by; draw_g = k0 + src;
      if (am == 0u) flags |= 2;
      else if ((nm >> src) & 1u) flags |= 4;
      act = false;
    }
    tries += __popc(nm);
    k0 += GW;
  }

  if (!on) return;
  // start, goal (B,1,4) = [x, y, 0, 0]; draws, info
  IO* so = (IO*)a.start + b * 4;
  IO* go = (IO*)a.goal + b * 4;
  if (l < 4) so[l] = (IO)(l == 0 ? sx : (l == 1 ? sy : 0.0));
  else if (l < 8) go[l - 4] = (IO)(l == 4 ? gx : (l == 5 ? gy : 0.0));
  else if (l == 8) { if (a.draws != nullptr) a.draws[b * 2] = draw_s; }
  else if (l == 9) { if (a.draws != nullptr) a.draws[b * 2 + 1] = draw_g; }
  else if (l == 10) { if (a.info != nullptr) a.info[b] = flags; }
  // straight_line_trajb (utils/planner_utils.py:47-56): element e = 4 i + c of the problem's (n, 4) block, adjacent lanes adjacent elements
  const int n = p.n, N = n - 1;
  const double Nd = (double)N;
  IO* th = (IO*)a.th_init + b * (int64_t)n * 4;
  for (int e = l; e < n * 4; e += GW) {
    const int i = e >> 2, c = e & 3;
    const double s = (c & 1) ? sy : sx, g = (c & 1) ? gy : gx;
    const double pos = s * (double)(N - i) * 1.0 / Nd * 1.0 + g * (double)i * 1.0 / Nd * 1.0;
    const double vel = (g - s) / a.total_time_sec * 1.0;
    th[e] = (IO)(c < 2 ? pos : vel);
  }
}

}  // namespace

extern "C" int dgp_sample_problems(const DgpHandle* h, int32_t batch, const DgpSdf* sdf, const int32_t* env_index, const DgpSampleParams* sp, uint64_t seed,
                                   uint64_t first_problem, const int32_t* diagonal, void* start, void* goal, void* th_init, int32_t* draws, int32_t* info,
                                   void* stream) {
#pragma clang fp contract(off)
  const dgp_dev::Events ev = dgp_dev::take_events();
  if (!h) return fail(DGP_EINVAL, "null handle");
  if (h->cfg.dof != 2) return fail(DGP_EINVAL, "dgp_sample_problems: only dof == 2 (the reference samples 2-D point-robot problems only), got %d", h->cfg.dof);
  if (!sp) return fail(DGP_EINVAL, "dgp_sample_problems: null DgpSampleParams");
  if (!start || !goal || !th_init) return fail(DGP_EINVAL, "dgp_sample_problems: start, goal and th_init must be non-null device pointers");
  SampleArgs a;
  const int rc = dgp_host::fill_call(h, batch, th_init, start, goal, sdf, nullptr, a.p);
  if (rc != DGP_OK) return rc;
  if (sp->max_draws < 1) return fail(DGP_EINVAL, "dgp_sample_problems: max_draws must be >= 1, got %d", sp->max_draws);
  const DgpConfig& c = h->cfg;
  const double lbx = c.x_lims[0] + sp->margin, lby = c.y_lims[0] + sp->margin, ubx = c.x_lims[1] - sp->margin, uby = c.y_lims[1] - sp->margin;      // :58-61
  if (!(ubx > lbx) || !(uby > lby)) return fail(DGP_EINVAL, "dgp_sample_problems: margin %g leaves no sampling box inside the limits", sp->margin);
  if (!(sp->clearance == sp->clearance) || !(sp->min_dist_frac == sp->min_dist_frac) || !(sp->corner_inset == sp->corner_inset))
    return fail(DGP_EINVAL, "dgp_sample_problems: NaN in DgpSampleParams");
  a.env_index = env_index; a.diagonal = diagonal;
  a.start = start; a.goal = goal; a.th_init = th_init; a.draws = draws; a.info = info;
  a.first_problem = first_problem;
  a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32);
  a.near_tries = sp->near_tries; a.max_draws = sp->max_draws;
  a.clearance = sp->clearance;
  a.lbx = lbx; a.lby = lby; a.wx = ubx - lbx; a.wy = uby - lby;
  a.min_dist = sp->min_dist_frac * sqrt(a.wx * a.wx + a.wy * a.wy);      // 0.6 * max_d (:62, :77)
  a.max_d = c.x_lims[1] - c.x_lims[0];
  a.xlo = c.x_lims[0]; a.xhi = c.x_lims[1]; a.ylo = c.y_lims[0]; a.yhi = c.y_lims[1];
  a.cxlo = c.x_lims[0] + sp->corner_inset; a.cxhi = c.x_lims[1] - sp->corner_inset;      // :134-145
  a.cylo = c.y_lims[0] + sp->corner_inset; a.cyhi = c.y_lims[1] - sp->corner_inset;
  a.total_time_sec = c.total_time_sec;
  const dim3 grid((unsigned)((a.p.B + (64 / GW) - 1) / (64 / GW))), block(64);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = c.io_dtype == DGP_F64 ? dgp_dev::launch(sample_problems_kernel<double>, grid, block, 0, s, ev, a)
                                             : dgp_dev::launch(sample_problems_kernel<float>, grid, block, 0, s, ev, a);
  return dgp_dev::hip_rc(e, "dgp_sample_problems");
}
