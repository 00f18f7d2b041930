// dgp_dense_walk.h -- the dense check of one trajectory by the LPT lanes of its group, stated once for gp_interpolate.hip (dgp_gp_interpolate) and
// select_samples.hip (dgp_select_samples): the per-lane strided walk over the dense index m = lane + k LPT -- the header's closed form and operation order, the
// obstacle lookup (gn_lane.h's obstacle_eval) at the UNROUNDED fp64 position, the lane's partial sum / maximum with its index / count / first index -- and the four
// butterfly reductions over the group (dgp_group.h's, and the maximum with its index below).  The order of every addition and comparison depends on N_d and LPT
// only, so both units give the same bits for a trajectory.  HIP only (the __shfl_xor butterflies); include after DGP_TL is defined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gn_lane.h"
#include "dgp_group.h"
#include "dgp_status.h"      // (include/dgpmp2_hip.h: DGP_DENSE_*)

#pragma clang fp contract(off)

namespace dgp_dense {

constexpr int NO_INDEX = 0x7fffffff;

using dgp_group::group_sum;
using dgp_group::group_sum_i;
using dgp_group::group_min_i;

// the maximum with its index: a NaN wins over every number (torch.max), the smaller index wins between equals (and between NaNs).
// Symmetric: both partners of an exchange end with the same pair.
template <int LPT>
__device__ __forceinline__ void group_argmax(double& v, int& idx) {
#pragma unroll
  for (int m = 1; m < LPT; m <<= 1) {
    const double ov = __shfl_xor(v, m);
    const int oi = __shfl_xor(idx, m);
    const bool vn = v != v, on = ov != ov;
    const bool greater = (on && !vn) || ov > v, equal = (on && vn) || ov == v;
    const bool take = greater || (equal && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
  }
}

// what a lane (after reduce(): the whole group) knows of its trajectory's dense states 1 .. N_d - 2
struct Partials {
  double s_pen, m_pen;      // sum and maximum of the hinge costs
  int m_idx, cnt, first;    // dense index of the maximum, count of cost != 0, smallest dense index with cost != 0
};

// the closed limits of the handle and what CHECK = true gathers on the way: a looked-up position outside them (a NaN is outside), a stored value that is not finite
struct Limits { double xlo, xhi, ylo, yhi; };
struct Flags { bool outside, nonfinite; };

// Lane l of the group walks the dense states m = l, l + LPT, ... of the trajectory th (n, D): th_dense / dense_cost rows where the pointers are non-null, the
// partials where `look` (the grid is read then only).  Row i + 1 is clamped to n - 1 for the load (unconditional loads); offset 0 is a bit copy of row i.
// CHECK: the position the lookup takes of EVERY dense state, the two end states included, against `lim`, and every stored value (each support row is the copied
// row of exactly one dense state) for finiteness.
template <int DOF, typename IO, int LPT, bool CHECK>
__device__ __forceinline__ void walk(const dgp::GnParams& p, const IO* th, const IO* grid, IO* dense, IO* ocost, bool look, double eps, int k1, int nd, int l,
                                     Partials& r, const Limits& lim, Flags& f) {
  constexpr int D = 2 * DOF;
  const int n = p.n;
  const double dt = p.dt, fk1 = (double)k1;
  double s_pen = 0.0, m_pen = -__builtin_huge_val();
  int m_idx = NO_INDEX, cnt = 0, first = NO_INDEX;
  for (int m = l; m < nd; m += LPT) {
    const int i = m / k1, j = m - i * k1;
    const int i1 = i + 1 < n ? i + 1 : n - 1;      // clamped: the last dense state is a copy (j == 0), the row is unused
    IO r0[D], r1[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { r0[c] = th[(int64_t)i * D + c]; r1[c] = th[(int64_t)i1 * D + c]; }
    // the eight coefficients, in the header's operation order
    const double s = (double)j / fk1;
    const double s2 = s * s;
    const double s3 = s2 * s;
    const double a0 = (1.0 - 3.0 * s2) + 2.0 * s3;
    const double a1 = dt * ((s - 2.0 * s2) + s3);
    const double a2 = 3.0 * s2 - 2.0 * s3;
    const double a3 = dt * (s3 - s2);
    const double b2 = (6.0 * (s - s2)) / dt;
    const double b0 = -b2;
    const double b1 = (1.0 - 4.0 * s) + 3.0 * s2;
    const double b3 = 3.0 * s2 - 2.0 * s;
    const bool copy = j == 0;
    double q[D];
#pragma unroll
    for (int c = 0; c < DOF; ++c) {
      const double x0 = (double)r0[c], v0 = (double)r0[DOF + c], x1 = (double)r1[c], v1 = (double)r1[DOF + c];
      q[c] = ((a0 * x0 + a1 * v0) + a2 * x1) + a3 * v1;
      q[DOF + c] = ((b0 * x0 + b1 * v0) + b2 * x1) + b3 * v1;
    }
    if (dense != nullptr) {
#pragma unroll
      for (int c = 0; c < D; ++c) dense[(int64_t)m * D + c] = copy ? r0[c] : (IO)q[c];      // a support state passes through untouched, bit for bit
    }
    const double px = copy ? (double)r0[0] : q[0], py = copy ? (double)r0[1] : q[1];
    if constexpr (CHECK) {
      f.outside = f.outside || !(px >= lim.xlo && px <= lim.xhi && py >= lim.ylo && py <= lim.yhi);
      if (copy) {
#pragma unroll
        for (int c = 0; c < D; ++c) {
          const double v = (double)r0[c];
          f.nonfinite = f.nonfinite || !(v - v == 0.0);
        }
      }
    }
    if (look) {
      double cost, hx, hy;
      dgp::obstacle_eval<IO>(p, grid, px, py, eps, cost, hx, hy);
      if (ocost != nullptr) ocost[m] = (IO)cost;
      const bool interior = m >= 1 && m < nd - 1;      // collision_metrics' convention: the first and the last state are left out
      s_pen += interior ? cost : 0.0;
      const bool hit = interior && cost != 0.0;        // torch.nonzero: a NaN counts
      cnt += hit ? 1 : 0;
      first = (hit && m < first) ? m : first;
      const bool take = interior && ((cost != cost && !(m_pen != m_pen)) || cost > m_pen);      // m rises: the smallest index of equals stays
      m_pen = take ? cost : m_pen;
      m_idx = take ? m : m_idx;
    }
  }
  r.s_pen = s_pen; r.m_pen = m_pen; r.m_idx = m_idx; r.cnt = cnt; r.first = first;
}

// the lanes' partials -> the trajectory's, on every lane of the group
template <int LPT>
__device__ __forceinline__ void reduce(Partials& r) {
  r.s_pen = group_sum<LPT>(r.s_pen);
  group_argmax<LPT>(r.m_pen, r.m_idx);
  r.cnt = group_sum_i<LPT>(r.cnt);
  r.first = group_min_i<LPT>(r.first);
}

// column `col` of the DGP_DENSE_* summary from the reduced partials
__device__ __forceinline__ double summary_column(int col, const Partials& r, int nd) {
  switch (col) {
    case DGP_DENSE_IN_COLL: return r.cnt > 0 ? 1.0 : 0.0;
    case DGP_DENSE_NUM_COLLIDING: return (double)r.cnt;
    case DGP_DENSE_AVG_PENETRATION: return r.s_pen / (double)(nd - 2);
    case DGP_DENSE_MAX_PENETRATION: return r.m_pen;
    case DGP_DENSE_FIRST_COLLIDING: return r.first == NO_INDEX ? -1.0 : (double)r.first;
    case DGP_DENSE_WORST_INDEX: return (double)r.m_idx;
    default: return 0.0;
  }
}

}  // namespace dgp_dense
