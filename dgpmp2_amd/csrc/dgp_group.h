// dgp_group.h -- what the LPT lanes that share one trajectory (or batch row) of a side kernel do together, stated once for every unit that maps a batch this way:
// the lanes-per-trajectory rule of the strided walks, the butterfly reductions and the inclusive scan over the group.
// HIP only (the __shfl_* exchanges), nothing of the solver.  No function here holds a multiply-add pair: each serves units with contraction on and off alike.
// A reduction or scan with one user stays in its unit (group_max, group_argmax, group_argmin, group_max_scan, group_mat_vec), and so does the opening of these
// kernels (l = lane % LPT, the group's trajectory b clamped to the last one, `on`): behind a function the kernels no longer compile to the code they are held to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgp_group {

// lanes per trajectory of a strided walk over `count` states / dense states / points: every lane has up to four of them before a wider group pays (one round of
// memory latency either way).  dgp_traj_metrics, dgp_gp_interpolate, dgp_select_samples, dgp_sdf_lookup.
inline int lanes_for(int count) { return count <= 64 ? 16 : (count <= 128 ? 32 : 64); }

template <int LPT>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int m = 1; m < LPT; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
template <int LPT>
__device__ __forceinline__ int group_sum_i(int v) {
#pragma unroll
  for (int m = 1; m < LPT; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
template <int LPT>
__device__ __forceinline__ int group_min_i(int v) {
#pragma unroll
  for (int m = 1; m < LPT; m <<= 1) {
    const int o = __shfl_xor(v, m);
    v = o < v ? o : v;
  }
  return v;
}

// inclusive Hillis-Steele scan over the LPT lanes of a group: x_l <- x_(l - off) + x_l for l >= off, off = 1, 2, 4, ...
template <int LPT>
__device__ __forceinline__ double group_scan(double x, int l) {
#pragma unroll
  for (int off = 1; off < LPT; off <<= 1) {
    const double lo = __shfl_up(x, off, LPT);
    x = l >= off ? lo + x : x;
  }
  return x;
}

}  // namespace dgp_group
