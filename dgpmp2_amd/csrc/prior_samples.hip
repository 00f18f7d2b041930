// prior_samples.hip -- dgp_prior_samples: S trajectories per problem drawn from the GP prior the solver uses as its smoothness model, conditioned on the start and goal
// priors, in ONE launch (gfx950 / CDNA4): the initial trajectories of a multi-start.
//
// What it builds: nothing the reference has -- it hands Gauss-Newton one initial trajectory per problem (straight_line_trajb, utils/planner_utils.py:47-56, or the RRT*
// path).  The law is N(mu, Sigma) with Sigma^-1 = A^T K^-1 A of the step kernels' system without obstacle, non-holonomic and velocity-limit rows and without reg, built
// the way every planner of the GPMP family samples it: the unconditioned constant-velocity chain from the start prior, one noisy observation of its last state, and
// Matheron's rule.  include/dgpmp2_hip.h states the construction and its fp64 operation order, tests/prior_oracle.py restates it, and the kernel is held against that
// bit for bit; dgp_prior.h forms the constants (Q_c, L_c, S^-1) on the host.
//
// Mapping: one trajectory (b, s) per group of LPT = 16 / 32 / 64 lanes (dgp_prior::launch_shape(n)), 64 / LPT trajectories per wavefront, lane l holds state l.  The
// chain is two additive prefix scans per dof component -- velocities, then positions -- run as Hillis-Steele steps over the group (__shfl_up: the cross-lane network,
// no LDS allocation, no barrier).  The association order is the header's: it depends on the state index alone, so a narrower group computes the same bits.  Past 64
// states (LONG) a wavefront walks blocks of 64 states with the carried last state added to each block's local scan, twice: the goal observation y needs the last state
// before any state can be conditioned, and keeping up to 16 blocks of states alive costs more registers than generating the noise again.
// Noise: lane l draws row l of the (n + 1, d) normals -- d / 2 Philox blocks, one Box-Muller pair each -- and the last row (the goal observation) is split over the
// first d / 2 lanes of the group and broadcast; supplied noise is read the same way.
// Stores: a lane stores its whole state row (16 / 24 / 32 / 48 bytes, as 8- or 16-byte vectors where the pointer allows), adjacent lanes adjacent rows: a wavefront
// writes one contiguous run of full lines.  No atomics, nothing allocated or synchronised.  Lane groups past the end of a ragged launch recompute the last trajectory
// and store nothing (no divergent shuffles).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dgp_prior.h"
#include "dgp_launch.h"
#include "dgp_philox.h"
#include "dgp_group.h"
#include "dgp_rowio.h"

#pragma clang fp contract(off)

namespace {

using dgp_host::fail;
using dgp_prior::PriorConsts;
using dgp_prior::PCoef;

struct PriorArgs {
  PriorConsts k;
  const void *start, *goal, *mean;      // (B,1,d), (B,1,d), (B,n,d) or null
  const double* noise;                  // (B,S,n+1,d) or null: generate
  void* th;                             // (B,S,n,d)
  double* noise_out;                    // (B,S,n+1,d) or null
  int32_t* info;                        // (B,S) or null
  int64_t T;                            // B * S trajectories
  int32_t S, n;
  uint64_t first_problem;
  uint32_t key0, key1;
  double scale;
  double xlo, xhi, ylo, yhi;
  int32_t vec;                          // th allows the vector stores of store_row
};
static_assert(sizeof(PriorArgs) <= 4096, "kernel-argument segment");

// Philox block j of trajectory (problem, s): normals 2 j and 2 j + 1 of its row-major (n + 1, d) array
__device__ __forceinline__ void normal_pair(const PriorArgs& a, uint64_t problem, uint32_t s, uint32_t j, double& z0, double& z1) {
  uint32_t w[4];
  dgp::philox4x32_10((uint32_t)problem, (uint32_t)(problem >> 32), j, (dgp_prior::kStreamTag << 24) | s, a.key0, a.key1, w);
  const double u0 = (double)((((uint64_t)w[0] << 32) | w[1]) >> 11) * 0x1.0p-53;
  const double u1 = (double)((((uint64_t)w[2] << 32) | w[3]) >> 11) * 0x1.0p-53;
  const double r = sqrt(-2.0 * log(1.0 - u0));
  const double ang = 6.283185307179586 * u1;
  z0 = r * cos(ang);
  z1 = r * sin(ang);
}

// row `row` of the trajectory's normals: generated, or read from `noise` (nz: the trajectory's (n + 1, d) block there)
template <int D>
__device__ __forceinline__ void noise_row(const PriorArgs& a, const double* nz, uint64_t problem, uint32_t s, int row, double (&z)[D]) {
  if (a.noise != nullptr) {
#pragma unroll
    for (int c = 0; c < D; ++c) z[c] = nz[(int64_t)row * D + c];
  } else {
#pragma unroll
    for (int i = 0; i < D / 2; ++i) normal_pair(a, problem, s, (uint32_t)(row * (D / 2) + i), z[2 * i], z[2 * i + 1]);
  }
}

using dgp_group::group_scan;
using dgp_rowio::store_row;

// W(t) g = P(t) Phi(t_end - t)^T g, g = S^-1 (an observation residual)
template <int DOF>
__device__ __forceinline__ void apply_w(const PriorConsts& k, double t, const double (&g)[2 * DOF], double (&out)[2 * DOF]) {
  const double tau = k.t_end - t;
  const PCoef pc = dgp_prior::p_coef(k.ks2, t);
  double hp[DOF], hv[DOF], ap[DOF], av[DOF];
#pragma unroll
  for (int c = 0; c < DOF; ++c) {
    hp[c] = g[c];
    hv[c] = tau * g[c] + g[DOF + c];
    ap[c] = pc.q_pp * hp[c] + pc.q_pv * hv[c];
    av[c] = pc.q_pv * hp[c] + pc.q_vv * hv[c];
  }
#pragma unroll
  for (int c = 0; c < DOF; ++c) {
    double qp = k.Qc[c * DOF] * ap[0], qv = k.Qc[c * DOF] * av[0];
#pragma unroll
    for (int j = 1; j < DOF; ++j) { qp = qp + k.Qc[c * DOF + j] * ap[j]; qv = qv + k.Qc[c * DOF + j] * av[j]; }
    out[c] = (pc.i_pp * hp[c] + pc.i_pv * hv[c]) + qp;
    out[DOF + c] = (pc.i_pv * hp[c] + k.ks2 * hv[c]) + qv;
  }
}

// y = M x for the uniform-per-group x, M (D x D) in the kernel-argument segment: lane i < D of the group forms row i -- its entries come through a vector load at
// a per-lane address, so the matrix never occupies scalar registers -- and the D results are broadcast.  Row i is summed left to right, as mat-vec products are everywhere.
template <int D>
__device__ __forceinline__ void group_mat_vec(const double* M, const double (&x)[D], int l, int gbase, double (&y)[D]) {
  const double* row = M + (l < D ? l : 0) * D;
  double s = row[0] * x[0];
#pragma unroll
  for (int j = 1; j < D; ++j) s = s + row[j] * x[j];
#pragma unroll
  for (int i = 0; i < D; ++i) y[i] = __shfl(s, gbase + i);
}

// The unconditioned chain over one block of LPT states starting at state k0: lane l gets x_(k0 + l) in (xp, xv) and its noise row in z.  carry_p / carry_v: the
// state k0 - 1 (read for k0 > 0 only).
template <int DOF, int LPT>
__device__ __forceinline__ void chain_block(const PriorArgs& a, const double* nz, uint64_t problem, uint32_t s, int k0, int l, const double (&carry_p)[DOF],
                                            const double (&carry_v)[DOF], double (&z)[2 * DOF], double (&xp)[DOF], double (&xv)[DOF]) {
  constexpr int D = 2 * DOF;
  const PriorConsts& k = a.k;
  const int st = k0 + l;
  const int row = st <= a.n ? st : a.n;      // (lanes past the last state: any row inside the array; their values reach no stored state)
  noise_row<D>(a, nz, problem, s, row, z);
  double ev[DOF], wp[DOF];
#pragma unroll
  for (int c = 0; c < DOF; ++c) {
    double lu = k.Lc[c * DOF] * z[0], lw = k.Lc[c * DOF] * z[DOF];
#pragma unroll
    for (int j = 1; j <= c; ++j) { lu = lu + k.Lc[c * DOF + j] * z[j]; lw = lw + k.Lc[c * DOF + j] * z[DOF + j]; }
    wp[c] = k.cp * lu;
    const double wv = k.cv1 * lu + k.cv2 * lw;
    ev[c] = st == 0 ? k.ks * z[DOF + c] : wv;
  }
#pragma unroll
  for (int c = 0; c < DOF; ++c) {
    double v = group_scan<LPT>(ev[c], l);
    if (k0 > 0) v = carry_v[c] + v;
    xv[c] = v;
    double vprev = __shfl_up(v, 1, LPT);
    if (l == 0) vprev = carry_v[c];
    const double ep = st == 0 ? k.ks * z[c] : wp[c] + k.dt * vprev;
    double p = group_scan<LPT>(ep, l);
    if (k0 > 0) p = carry_p[c] + p;
    xp[c] = p;
  }
}

template <int DOF, typename IO, int LPT, bool LONG>
__global__ void __launch_bounds__(64) prior_samples_kernel(const PriorArgs a) {
  constexpr int D = 2 * DOF, TPW = 64 / LPT;
  static_assert(!LONG || LPT == 64, "blocks of 64 states");
  const PriorConsts& k = a.k;
  const int lane = (int)threadIdx.x, l = lane % LPT, gbase = lane - l;
  const int64_t t_raw = (int64_t)blockIdx.x * TPW + lane / LPT;
  const bool on = t_raw < a.T;
  const int64_t t = on ? t_raw : a.T - 1;
  const int64_t b = t / a.S;
  const uint32_t s = (uint32_t)(t - b * a.S);
  const uint64_t problem = a.first_problem + (uint64_t)b;
  const int n = a.n;
  const double* nz = a.noise != nullptr ? a.noise + t * (int64_t)(n + 1) * D : nullptr;
  double* nzo = a.noise_out != nullptr ? a.noise_out + t * (int64_t)(n + 1) * D : nullptr;
  const IO* start = (const IO*)a.start + b * D;
  const IO* goal = (const IO*)a.goal + b * D;
  const IO* mean = a.mean != nullptr ? (const IO*)a.mean + b * (int64_t)n * D : nullptr;
  IO* th = (IO*)a.th + t * (int64_t)n * D;

  double carry_p[DOF], carry_v[DOF], z[D], xp[DOF], xv[DOF], gy[D], gr[D], sp[DOF], sv[DOF];
#pragma unroll
  for (int c = 0; c < DOF; ++c) { sp[c] = (double)start[c]; sv[c] = (double)start[DOF + c]; }
  const int last_k0 = LONG ? ((n - 1) / 64) * 64 : 0, last_l = (n - 1) - last_k0;      // the block and the lane of state n - 1 (not LONG: n <= LPT, block 0)
  bool outside = false, nonfinite = false;
  // LONG: pass 0 runs the chain alone, up to the goal observation; pass 1 runs it again and conditions.  Otherwise the one block does both in one trip.
  constexpr int OBSERVE = LONG ? 0 : 1;
  for (int pass = OBSERVE; pass < 2; ++pass) {
#pragma unroll
    for (int c = 0; c < DOF; ++c) carry_p[c] = carry_v[c] = 0.0;
    for (int k0 = 0; k0 <= last_k0; k0 += LPT) {
      chain_block<DOF, LPT>(a, nz, problem, s, k0, l, carry_p, carry_v, z, xp, xv);
      if constexpr (LONG) {
#pragma unroll
        for (int c = 0; c < DOF; ++c) { carry_p[c] = __shfl(xp[c], 63); carry_v[c] = __shfl(xv[c], 63); }
      }
      if (pass == OBSERVE && k0 == last_k0) {
        // the goal observation y = x_(n-1) + K_g z_g: row n of the normals, two entries per lane on the first DOF lanes of the group
        double g0, g1, zg[D], y[D], r0[D];
        const int i = l < DOF ? l : DOF - 1;
        if (a.noise != nullptr) { g0 = nz[(int64_t)n * D + 2 * i]; g1 = nz[(int64_t)n * D + 2 * i + 1]; }
        else normal_pair(a, problem, s, (uint32_t)(n * DOF + i), g0, g1);
        if (nzo != nullptr && on && l < DOF) { nzo[(int64_t)n * D + 2 * l] = g0; nzo[(int64_t)n * D + 2 * l + 1] = g1; }
#pragma unroll
        for (int c = 0; c < DOF; ++c) { zg[2 * c] = __shfl(g0, gbase + c); zg[2 * c + 1] = __shfl(g1, gbase + c); }
#pragma unroll
        for (int c = 0; c < DOF; ++c) {
          y[c] = __shfl(xp[c], gbase + last_l) + k.kg * zg[c];
          y[DOF + c] = __shfl(xv[c], gbase + last_l) + k.kg * zg[DOF + c];
          r0[c] = (double)goal[c] - (sp[c] + k.t_end * sv[c]);
          r0[DOF + c] = (double)goal[DOF + c] - sv[c];
        }
        group_mat_vec<D>(k.Sinv, y, l, gbase, gy);
        group_mat_vec<D>(k.Sinv, r0, l, gbase, gr);
      }
      if (pass == 0) continue;
      const int st = k0 + l;
      const bool live = on && st < n;
      const int sr = st < n ? st : n - 1;      // (clamped for the loads)
      const double tk = (double)sr * k.dt;
      double wy[D], m[D];
      apply_w<DOF>(k, tk, gy, wy);
      if (mean != nullptr) {
#pragma unroll
        for (int c = 0; c < D; ++c) m[c] = (double)mean[(int64_t)sr * D + c];
      } else {
        double wr[D];
        apply_w<DOF>(k, tk, gr, wr);
#pragma unroll
        for (int c = 0; c < DOF; ++c) { m[c] = (sp[c] + tk * sv[c]) + wr[c]; m[DOF + c] = sv[c] + wr[DOF + c]; }
      }
      IO q[D];
#pragma unroll
      for (int c = 0; c < DOF; ++c) {
        q[c] = (IO)(m[c] + a.scale * (xp[c] - wy[c]));
        q[DOF + c] = (IO)(m[DOF + c] + a.scale * (xv[c] - wy[DOF + c]));
      }
      if (live) {
        store_row<IO, D>(th + (int64_t)st * D, q, a.vec != 0);
        if (nzo != nullptr) {
#pragma unroll
          for (int c = 0; c < D; ++c) nzo[(int64_t)st * D + c] = z[c];
        }
        const double qx = (double)q[0], qy = (double)q[1];
        outside = outside || !(qx >= a.xlo && qx <= a.xhi && qy >= a.ylo && qy <= a.yhi);
#pragma unroll
        for (int c = 0; c < D; ++c) {
          const double v = (double)q[c];
          nonfinite = nonfinite || !(v - v == 0.0);
        }
      }
    }
  }
  const uint64_t gmask = (~0ull >> (64 - LPT)) << gbase;
  const bool any_out = (__ballot(outside) & gmask) != 0ull, any_nf = (__ballot(nonfinite) & gmask) != 0ull;
  if (a.info != nullptr && on && l == 0) a.info[t] = (any_out ? 1 : 0) | (any_nf ? 2 : 0);
}

template <int DOF, typename IO>
hipError_t launch_n(const PriorArgs& a, hipStream_t s, const dgp_dev::Events& ev) {
  const dgp_prior::LaunchShape sh = dgp_prior::launch_shape(a.n);
  const int tpw = 64 / sh.lpt;
  const dim3 grid((unsigned)((a.T + tpw - 1) / tpw)), block(64);
  if (sh.blocks > 1) return dgp_dev::launch(prior_samples_kernel<DOF, IO, 64, true>, grid, block, 0, s, ev, a);
  return dgp_dev::with_lpt(sh.lpt, [&](auto L) { return dgp_dev::launch(prior_samples_kernel<DOF, IO, L, false>, grid, block, 0, s, ev, a); });
}

}  // namespace

extern "C" int dgp_prior_samples(const DgpHandle* h, int32_t batch, int32_t num_samples, const void* start, const void* goal, const void* mean, double scale,
                                 uint64_t seed, uint64_t first_problem, const double* noise, void* th, double* noise_out, int32_t* info, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  if (!h) return fail(DGP_EINVAL, "null handle");
  const DgpConfig& c = *reinterpret_cast<const DgpConfig*>(h);      // DgpHandle's first member (dgp_host.h holds that with a static_assert); this unit needs nothing else of it
  if (!start || !goal || !th) return fail(DGP_EINVAL, "dgp_prior_samples: start, goal and th must be non-null device pointers");
  if (batch < 1) return fail(DGP_EINVAL, "dgp_prior_samples: batch must be positive, got %d", batch);
  if (num_samples < 1 || num_samples > dgp_prior::kMaxSamples)
    return fail(DGP_EINVAL, "dgp_prior_samples: num_samples must be in 1..%d (the sample index shares a counter word with the stream tag), got %d", dgp_prior::kMaxSamples,
                num_samples);
  if ((int64_t)batch * num_samples > (int64_t)0x7fffffff)
    return fail(DGP_EINVAL, "dgp_prior_samples: batch * num_samples = %lld trajectories exceed one launch (2^31 - 1)", (long long)batch * num_samples);
  if (!(scale >= 0.0) || !(scale < HUGE_VAL)) return fail(DGP_EINVAL, "dgp_prior_samples: scale must be finite and >= 0, got %g", scale);
  PriorArgs a;
  const int rc = dgp_prior::fill_consts(c, a.k);
  if (rc != DGP_OK) return rc;
  a.start = start; a.goal = goal; a.mean = mean; a.noise = noise; a.th = th; a.noise_out = noise_out; a.info = info;
  a.T = (int64_t)batch * num_samples; a.S = num_samples; a.n = c.num_states;
  a.first_problem = first_problem;
  a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32);
  a.scale = scale;
  a.xlo = c.x_lims[0]; a.xhi = c.x_lims[1]; a.ylo = c.y_lims[0]; a.yhi = c.y_lims[1];
  const bool f64 = c.io_dtype == DGP_F64;
  const uintptr_t need = (f64 || c.dof == 2) ? 15u : 7u;      // rows of 16 / 32 / 48 bytes move as 16-byte vectors, the 24-byte rows of dof 3 fp32 as 8-byte ones
  a.vec = (reinterpret_cast<uintptr_t>(th) & need) == 0 ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = dgp_dev::with_dof_io(c.dof, f64, [&](auto dof, auto io) { return launch_n<dof, decltype(io)>(a, s, ev); });
  return dgp_dev::hip_rc(e, "dgp_prior_samples");
}

extern "C" int dgp_prior_launch_shape(const DgpHandle* h, int32_t* lanes_per_traj, int32_t* blocks) {
  if (!h) return fail(DGP_EINVAL, "null handle");
  const dgp_prior::LaunchShape sh = dgp_prior::launch_shape(reinterpret_cast<const DgpConfig*>(h)->num_states);
  if (lanes_per_traj) *lanes_per_traj = sh.lpt;
  if (blocks) *blocks = sh.blocks;
  return DGP_OK;
}
