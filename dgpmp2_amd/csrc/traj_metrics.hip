// traj_metrics.hip -- dgp_traj_metrics: the validation metrics of a batch of planned trajectories in ONE launch (gfx950 / CDNA4).
//
// What it replaces: the metrics block the reference runs per trajectory after planning (learning/test_planner.py:299-334, datasets/test_dataset_sensitivity.py:175-206):
// gpfactor.get_error, obsfactor.get_error (built with eps = 0.0, test_planner.py:140), smoothness_metrics / collision_metrics (utils/planner_utils.py:75-102), the
// velocity-limit count (:310-322) and three MSELoss calls -- some thirty small torch kernels and a nonzero() (a device -> host synchronisation) per trajectory.
// include/dgpmp2_hip.h states every definition, quirks included.
//
// Mapping: LPT = 16 / 32 / 64 lanes per trajectory (n <= 64 / <= 128 / longer), 64 / LPT trajectories per wavefront, the states of a trajectory walked by its lanes
// in a strided loop (state i = lane + k LPT: adjacent lanes read adjacent rows of th, th_opt and write adjacent entries of obs_error), for every n and dof a handle accepts.
// The neighbour rows of the first and second differences (x_{i+1}, x_{i+2}) are RE-READ -- they are the rows the neighbouring lanes load in the same instruction, so the
// lines are in flight or in the vector L1 already; the kernel moves some 4 MB at B = 4096, n = 64 and is bound by the launch and one round of memory latency, not by bandwidth.
// The obstacle lookup is gn_lane.h's obstacle_eval (fp64 operation order of the reference, contraction off, clamped indices, `<=` hinge): a state has a hinge error here
// exactly when the step kernels give it one at the same epsilon.  DGP_TL = 2 (this unit's flag): the grid layout is a run-time branch, one kernel for both layouts.
// Reduction: every lane keeps fp64 partial sums / a maximum / two counts of its states, then a butterfly over the trajectory's LPT lanes (ds_bpermute) -- a fixed order that
// depends on n and LPT only: no atomics, bit-identical results from run to run and wherever the trajectory sits in the batch.  Lanes 0 .. 12 of a trajectory store its
// DGP_METRIC_COUNT doubles as one contiguous run.  Lane groups past the end of a ragged batch recompute the last trajectory and store nothing (no divergent shuffles).
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifndef DGP_TL
#define DGP_TL 2
#endif
#include "dgp_host.h"
#include "dgp_launch.h"
#include "dgp_group.h"

namespace {

using dgp_host::fail;

struct MetricsArgs {
  dgp::GnParams p;         // B, n, th, the grid and the constants of the bilinear lookup (dgp_host::fill_call); flags, vmax, dt
  const void* th_opt;      // (B, n, d) or null
  double* metrics;         // (B, DGP_METRIC_COUNT) or null
  void* obs_error;         // (B, n) or null
  double eps;              // metric_eps
  double total_time_sec;
};
static_assert(sizeof(MetricsArgs) <= 4096, "kernel-argument segment");

using dgp_group::group_sum;
using dgp_group::group_sum_i;

// torch.max: a NaN wins
__device__ __forceinline__ double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }
template <int LPT>
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
  for (int m = 1; m < LPT; m <<= 1) {
    const double o = __shfl_xor(v, m);
    v = (v != v) ? v : max_nan(v, o);      // (symmetric: both partners end with the same value)
  }
  return v;
}

template <int D, typename IO>
__device__ __forceinline__ void load_row(const IO* __restrict__ r, double (&x)[D]) {
#pragma unroll
  for (int c = 0; c < D; ++c) x[c] = (double)r[c];
}

template <int DOF, typename IO, int LPT>
__global__ void __launch_bounds__(64) traj_metrics_kernel(const MetricsArgs a) {
  constexpr int D = 2 * DOF, TPW = 64 / LPT;
  const dgp::GnParams& p = a.p;
  const int lane = (int)threadIdx.x, l = lane % LPT;
  const int64_t b_raw = (int64_t)blockIdx.x * TPW + lane / LPT;
  const bool on = b_raw < p.B;
  const int64_t b = on ? b_raw : (int64_t)p.B - 1;
  const int n = p.n;
  const IO* th = (const IO*)p.th + b * n * D;
  const IO* opt = (a.th_opt != nullptr ? (const IO*)a.th_opt : (const IO*)p.th) + b * n * D;      // no expert trajectory: th against itself, the three MSEs are exact zeros
  const IO* grid = (const IO*)p.sdf + b * p.sdf_bstride;
  IO* oerr = (IO*)a.obs_error + b * n;
  const bool limits = (p.flags & dgp::FLAG_VEL_LIMITS) != 0;
  double s_vel = 0.0, s_acc = 0.0, s_jerk = 0.0, s_gp = 0.0, s_pen = 0.0, s_pos = 0.0, s_velmse = 0.0;
  double m_pen = -__builtin_huge_val();
  int cnt = 0, viol = 0;
  for (int i = l; i < n; i += LPT) {
    const int i1 = i + 1 < n ? i + 1 : n - 1, i2 = i + 2 < n ? i + 2 : n - 1;      // clamped: the differences they feed are masked below
    double x0[D], x1[D], x2[D], xo[D];
    load_row<D, IO>(th + (int64_t)i * D, x0);
    load_row<D, IO>(th + (int64_t)i1 * D, x1);
    load_row<D, IO>(th + (int64_t)i2 * D, x2);
    load_row<D, IO>(opt + (int64_t)i * D, xo);
    // raw obstacle error of the state (obstacle_factor.py:35-40 at eps = metric_eps)
    double cost, hx, hy;
    dgp::obstacle_eval<IO>(p, grid, x0[0], x0[1], a.eps, cost, hx, hy);
    if (a.obs_error != nullptr && on) oerr[i] = (IO)cost;
    const bool interior = i >= 1 && i < n - 1;                                     // collision_metrics drops the first and the last state (planner_utils.py:93)
    s_pen += interior ? cost : 0.0;
    m_pen = interior ? max_nan(m_pen, cost) : m_pen;
    cnt += (interior && cost != 0.0) ? 1 : 0;                                      // torch.nonzero: NaN counts
    // smoothness_metrics (planner_utils.py:75-90): columns 2.. of the rows, of their first and of their second differences
    double v2 = 0.0, a2 = 0.0, j2 = 0.0, g2 = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const double d0 = x1[c] - x0[c], d1 = x2[c] - x1[c];
      const double dd = d1 - d0;
      if (c >= 2) { v2 += x0[c] * x0[c]; a2 += d0 * d0; j2 += dd * dd; }
      // GP factor error e = x_{i+1} - Phi x_i, Phi = [[I, dt I], [0, I]] (gp_factor.py)
      const double e = c < DOF ? x1[c] - (x0[c] + p.dt * x0[DOF + c]) : d0;
      g2 += e * e;
    }
    s_vel += sqrt(v2);
    s_acc += i + 1 < n ? sqrt(a2) : 0.0;
    s_gp += i + 1 < n ? g2 : 0.0;
    s_jerk += i + 2 < n ? sqrt(j2) : 0.0;
    // velocity-limit count (test_planner.py:314-320): state columns 2 and 3 whatever dof
    viol += (limits && !(fabs(x0[2]) <= p.vmax[0] && fabs(x0[3]) <= p.vmax[1])) ? 1 : 0;
    // MSELoss against the expert trajectory: positions, velocities
    double ep = 0.0, ev = 0.0;
#pragma unroll
    for (int c = 0; c < DOF; ++c) {
      const double dp = x0[c] - xo[c], dv = x0[DOF + c] - xo[DOF + c];
      ep += dp * dp; ev += dv * dv;
    }
    s_pos += ep; s_velmse += ev;
  }
  s_vel = group_sum<LPT>(s_vel); s_acc = group_sum<LPT>(s_acc); s_jerk = group_sum<LPT>(s_jerk); s_gp = group_sum<LPT>(s_gp);
  s_pen = group_sum<LPT>(s_pen); s_pos = group_sum<LPT>(s_pos); s_velmse = group_sum<LPT>(s_velmse);
  m_pen = group_max<LPT>(m_pen);
  cnt = group_sum_i<LPT>(cnt); viol = group_sum_i<LPT>(viol);
  if (a.metrics == nullptr) return;
  const double steps = (double)(n - 1), nn = (double)n;
  double out;
  switch (l) {
    case DGP_METRIC_AVG_VEL: out = s_vel / nn; break;
    case DGP_METRIC_AVG_ACC: out = s_acc / steps / steps; break;                        // rows / total_time_step, mean over n - 1 rows
    case DGP_METRIC_AVG_JERK: out = s_jerk / (steps * steps) / (double)(n - 2); break;  // rows / total_time_step^2, mean over n - 2 rows
    case DGP_METRIC_GP_MSE: out = s_gp / (steps * (double)D); break;
    case DGP_METRIC_IN_COLL: out = cnt > 0 ? 1.0 : 0.0; break;
    case DGP_METRIC_NUM_PENETRATING: out = (double)cnt; break;
    case DGP_METRIC_AVG_PENETRATION: out = s_pen / (double)(n - 2); break;
    case DGP_METRIC_MAX_PENETRATION: out = m_pen; break;
    case DGP_METRIC_COLL_INTENSITY: out = ((1.5 * (double)cnt) * p.dt) / a.total_time_sec; break;      // numel(nonzero of an (n-2,1,1) tensor) / 2 = 1.5 count (planner_utils.py:94-100)
    case DGP_METRIC_CONSTRAINT_VIOLATION: out = (double)viol / nn; break;
    case DGP_METRIC_POS_MSE: out = s_pos / (nn * (double)DOF); break;
    case DGP_METRIC_VEL_MSE: out = s_velmse / (nn * (double)DOF); break;
    case DGP_METRIC_TRAJ_MSE: out = (s_pos + s_velmse) / (nn * (double)D); break;
    default: out = 0.0; break;
  }
  if (on && l < DGP_METRIC_COUNT) a.metrics[b * DGP_METRIC_COUNT + l] = out;
}

}  // namespace

extern "C" int dgp_traj_metrics(const DgpHandle* h, int32_t batch, const void* th, const DgpSdf* sdf, double metric_eps, const void* th_opt,
                                double* metrics, void* obs_error, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  MetricsArgs a;
  const int rc = dgp_host::fill_call(h, batch, th, /*start=*/th, /*goal=*/th, sdf, nullptr, a.p);      // (no start / goal here: th stands in for the null checks)
  if (rc != DGP_OK) return rc;
  if (!metrics && !obs_error) return fail(DGP_EINVAL, "dgp_traj_metrics: metrics and obs_error are both null");
  if (metrics && a.p.n < 3) return fail(DGP_EINVAL, "dgp_traj_metrics: the metrics need num_states >= 3 (no interior state), got %d", a.p.n);
  a.th_opt = th_opt; a.metrics = metrics; a.obs_error = obs_error;
  a.eps = metric_eps; a.total_time_sec = h->cfg.total_time_sec;
  const int lpt = dgp_group::lanes_for(a.p.n), tpw = 64 / lpt;
  const dim3 grid((unsigned)((a.p.B + tpw - 1) / tpw)), block(64);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = dgp_dev::with_dof_io(h->cfg.dof, h->cfg.io_dtype == DGP_F64, [&](auto dof, auto io) {
    return dgp_dev::with_lpt(lpt, [&](auto L) { return dgp_dev::launch(traj_metrics_kernel<dof, decltype(io), L>, grid, block, 0, s, ev, a); });
  });
  return dgp_dev::hip_rc(e, "dgp_traj_metrics");
}
