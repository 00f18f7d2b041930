// gp_interpolate.hip -- dgp_gp_interpolate: the GP-interpolated dense trajectory of every trajectory of a batch, the hinge cost of every dense state and a
// collision summary over them, in ONE launch (gfx950 / CDNA4).
//
// What it builds: the capability the reference names and never implements -- gpmp2_planner.py:29-41 reads planner_params['total_check_step'] / ['use_gp_inter'], derives
// check_inter and sizes num_obs_factors for it, examples/gpmp2_xyh_params.yaml:7-8 carries the keys, and no code interpolates anything.  The rule is GPMP2's: the posterior
// mean of the constant-velocity prior between two support states, Lambda(tau) theta_i + Psi(tau) theta_{i+1} with Phi, Q, Q^-1 of gp/gp_factor.py:31-53; Q_c cancels, so
// one rule serves every covariance mode.  include/dgpmp2_hip.h states the closed form and its operation order, tests/interp_oracle.py restates it, and the kernel is held
// against that bit for bit.
//
// Mapping: LPT = 16 / 32 / 64 lanes per trajectory, chosen from the number of DENSE states N_d = (n - 1)(K + 1) + 1 (dgp_group::lanes_for), 64 / LPT trajectories per
// wavefront.  The lanes of a trajectory walk the dense index in a strided loop, m = lane + k LPT: adjacent lanes store adjacent rows of th_dense and adjacent entries of
// dense_cost (coalesced runs) and read the same or neighbouring support rows i = m / (K + 1), i + 1 -- the lines are in flight or in the vector L1 already, as for the
// neighbour rows of traj_metrics.hip.  Row i + 1 is clamped to n - 1 for the load (unconditional loads); the copy rule (offset 0 is a bit copy of row i) leaves the
// clamped row unused.  The obstacle lookup is gn_lane.h's obstacle_eval at the UNROUNDED fp64 position: a dense state has a hinge cost exactly where a support state at
// that position would in the step and metrics kernels.  DGP_TL = 2 (this unit's flag): the grid layout is a run-time branch, one kernel for both layouts.
// Reduction: every lane keeps an fp64 partial sum, a maximum with its index, a count and a minimum first index of its dense states, then a butterfly over the
// trajectory's LPT lanes -- a fixed order that depends on N_d and LPT only: no atomics, no LDS, bit-identical results from run to run, for either grid layout and
// wherever the trajectory sits in the batch.  Lanes 0 .. 5 of a trajectory store its DGP_DENSE_COUNT doubles as one contiguous run.  Lane groups past the end of a
// ragged batch recompute the last trajectory and store nothing (no divergent shuffles).  The walk and the reductions live in dgp_dense_walk.h, shared with
// select_samples.hip (dgp_select_samples), whose per-sample summary is this kernel's bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifndef DGP_TL
#define DGP_TL 2
#endif
#include "dgp_host.h"
#include "dgp_launch.h"
#include "dgp_dense_walk.h"

#pragma clang fp contract(off)

namespace {

using dgp_host::fail;

struct InterpArgs {
  dgp::GnParams p;         // B, n, th, the grid and the constants of the bilinear lookup (dgp_host::fill_call); dt
  void* th_dense;          // (B, N_d, d) or null
  void* dense_cost;        // (B, N_d) or null
  double* summary;         // (B, DGP_DENSE_COUNT) or null
  double eps;
  int32_t k1;              // num_inter + 1: dense states per interval
  int32_t nd;              // N_d
};
static_assert(sizeof(InterpArgs) <= 4096, "kernel-argument segment");

template <int DOF, typename IO, int LPT>
__global__ void __launch_bounds__(64) gp_interpolate_kernel(const InterpArgs a) {
  constexpr int D = 2 * DOF, TPW = 64 / LPT;
  const dgp::GnParams& p = a.p;
  const int lane = (int)threadIdx.x, l = lane % LPT;
  const int64_t b_raw = (int64_t)blockIdx.x * TPW + lane / LPT;
  const bool on = b_raw < p.B;
  const int64_t b = on ? b_raw : (int64_t)p.B - 1;
  const int n = p.n, k1 = a.k1, nd = a.nd;
  const IO* th = (const IO*)p.th + b * n * D;
  const IO* grid = (const IO*)p.sdf + b * p.sdf_bstride;      // (null without a cost / summary output: not read then)
  IO* dense = (IO*)a.th_dense + b * nd * D;
  IO* ocost = (IO*)a.dense_cost + b * nd;
  const bool look = a.dense_cost != nullptr || a.summary != nullptr;      // wave-uniform
  dgp_dense::Partials r;
  dgp_dense::Flags unused = {false, false};
  dgp_dense::walk<DOF, IO, LPT, false>(p, th, grid, (a.th_dense != nullptr && on) ? dense : nullptr, (a.dense_cost != nullptr && on) ? ocost : nullptr, look, a.eps, k1, nd, l,
                                       r, dgp_dense::Limits{0.0, 0.0, 0.0, 0.0}, unused);      // (dgp_dense_walk.h: shared with dgp_select_samples, the same bits)
  if (a.summary == nullptr) return;
  dgp_dense::reduce<LPT>(r);
  const double out = dgp_dense::summary_column(l, r, nd);
  if (on && l < DGP_DENSE_COUNT) a.summary[b * DGP_DENSE_COUNT + l] = out;
}

}  // namespace

extern "C" int dgp_gp_interpolate(const DgpHandle* h, int32_t batch, const void* th, int32_t num_inter, const DgpSdf* sdf, double eps,
                                  void* th_dense, void* dense_cost, double* summary, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  InterpArgs a;
  const int rc = dgp_host::fill_call(h, batch, th, /*start=*/th, /*goal=*/th, sdf, nullptr, a.p, /*sdf_optional=*/true);      // (no start / goal here: th stands in for the null checks)
  if (rc != DGP_OK) return rc;
  if (!th_dense && !dense_cost && !summary) return fail(DGP_EINVAL, "dgp_gp_interpolate: th_dense, dense_cost and summary are all null");
  if ((dense_cost || summary) && (!sdf || !sdf->data)) return fail(DGP_EINVAL, "dgp_gp_interpolate: dense_cost and summary need the signed-distance grid (sdf)");
  if (num_inter < 0 || num_inter > dgp_host::kMaxNumInter)
    return fail(DGP_EINVAL, "dgp_gp_interpolate: num_inter must be in 0..%d, got %d", dgp_host::kMaxNumInter, num_inter);
  a.k1 = num_inter + 1;
  a.nd = dgp_host::dense_states(a.p.n, num_inter);
  if (summary && a.nd < 3) return fail(DGP_EINVAL, "dgp_gp_interpolate: the summary needs at least 3 dense states (no interior state), got %d", a.nd);
  a.th_dense = th_dense; a.dense_cost = dense_cost; a.summary = summary; a.eps = eps;
  const int lpt = dgp_group::lanes_for(a.nd), tpw = 64 / lpt;
  const dim3 grid((unsigned)((a.p.B + tpw - 1) / tpw)), block(64);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = dgp_dev::with_dof_io(h->cfg.dof, h->cfg.io_dtype == DGP_F64, [&](auto dof, auto io) {
    return dgp_dev::with_lpt(lpt, [&](auto L) { return dgp_dev::launch(gp_interpolate_kernel<dof, decltype(io), L>, grid, block, 0, s, ev, a); });
  });
  return dgp_dev::hip_rc(e, "dgp_gp_interpolate");
}
