// step_loss.hip -- dgp_step_loss / dgp_step_loss_backward: the loss of one training iteration and its gradient (gfx950 / CDNA4).
//
// What it replaces: one_step_loss of the reference's training loop (learning/train_planner.py:75-120, called at :328) -- eight index_select, four cat, two einsum,
// five mean and the scalar arithmetic around them, some fifteen small kernels forward and at least as many backward, between the step launch and its backward
// launch.  include/dgpmp2_hip.h states every definition and its fp64 operation order, tests/loss_oracle.py restates it.
//
// Forward, launch 1 (loss_rows): LPT = 16 / 32 / 64 lanes per trajectory (n <= 16 / <= 32 / longer), 64 / LPT trajectories per wavefront.  The lanes of a trajectory
// walk its states in a strided loop, row i = lane + k LPT: adjacent lanes read adjacent rows of update, target and target_sub -- one row is d elements, 16 to 48
// bytes, fetched as 16-byte vectors (8-byte ones for the 24-byte rows of d = 6 in fp32) where every pointer of the call is aligned to the vector, element by element
// otherwise: the load width is the only difference, the arithmetic and its order are the same.  Every lane keeps two fp64 partial sums (position and velocity
// columns, row by row, column by column), then a butterfly over the trajectory's LPT lanes -- a fixed order that depends on n and LPT only.  Lanes 0 .. 4 of a
// trajectory store its DGP_LOSS_PER_TRAJ doubles as one contiguous run.  Lane groups past the end of a ragged batch recompute the last trajectory and store
// nothing (no divergent shuffles).
// Forward, launch 2 (loss_batch): ONE workgroup of 1024 lanes, stream-ordered behind launch 1.  Lane t sums rows t, t + 1024, ... of per_traj, a butterfly over the
// 64 lanes of a wavefront, the sixteen wavefront sums through LDS, added in wavefront order by lane 0, which forms the eight terms.  Store-and-sum instead of
// atomics: the sum has one order, the bits are the same from run to run.
// Backward (loss_backward): element-wise, one lane per row of (B n) in a grid-stride loop, the same row loads, up to three row stores; the first B lanes also
// store the three error gradients.  The cotangent is read from device memory: nothing crosses to the host.
// Both passes stream three (B, n, d) arrays once: HBM-bound byte kernels, 64-bit indices throughout (B n d may pass 2^31).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dgp_status.h"
#include "dgp_launch.h"
#include "dgp_group.h"
#include "dgp_rowio.h"

#pragma clang fp contract(off)

namespace {

using dgp_host::fail;

struct LossArgs {
  const void *update, *target, *target_sub;      // (B, n, d); target_sub may be null
  const void *unw_sg, *unw_gp, *unw_obs;         // (B) or null
  double* per_traj;                              // (B, DGP_LOSS_PER_TRAJ)
  double* terms;                                 // (DGP_LOSS_COUNT)
  DgpLossWeights w;
  int32_t B, n;
};

struct LossBwdArgs {
  const void *update, *target, *target_sub;
  const double* g_total;                         // device scalar or null (1.0)
  void *g_update, *g_target, *g_target_sub;      // (B, n, d) or null
  void *g_unw_sg, *g_unw_gp, *g_unw_obs;         // (B) or null
  DgpLossWeights w;
  int32_t B, n;
};

constexpr int kBatchLanes = 1024;                // loss_batch's workgroup
constexpr int kBwdLanes = 256;
constexpr int kBwdMaxBlocks = 1 << 16;           // the rest of the rows in the grid-stride loop

using dgp_group::group_sum;
using dgp_rowio::vec_bytes;

// dgp_rowio.h's rule and accesses in this unit's own wording (ext_vector_type, VEC a template flag): through dgp_rowio's load_row / store_row the sixteen vector
// kernels here compile to other code, and loss_rows<2, double, 16> then measured one 40 ns event tick above the range of this code's own repeated medians.
template <typename IO, int D, bool VEC>
__device__ __forceinline__ void load_row(const IO* p, IO (&r)[D]) {
  if (VEC) {
    constexpr int VE = vec_bytes<IO, D>() / (int)sizeof(IO);
    typedef IO vec_t __attribute__((ext_vector_type(VE)));
#pragma unroll
    for (int j = 0; j < D / VE; ++j) {
      const vec_t v = ((const vec_t*)p)[j];
#pragma unroll
      for (int e = 0; e < VE; ++e) r[j * VE + e] = v[e];
    }
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) r[c] = p[c];
  }
}

template <typename IO, int D, bool VEC>
__device__ __forceinline__ void store_row(IO* p, const IO (&r)[D]) {
  if (VEC) {
    constexpr int VE = vec_bytes<IO, D>() / (int)sizeof(IO);
    typedef IO vec_t __attribute__((ext_vector_type(VE)));
#pragma unroll
    for (int j = 0; j < D / VE; ++j) {
      vec_t v;
#pragma unroll
      for (int e = 0; e < VE; ++e) v[e] = r[j * VE + e];
      ((vec_t*)p)[j] = v;
    }
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) p[c] = r[c];
  }
}

// the per-element miss of one row, in the header's order; sub == null: no target_sub array (m = update - target)
template <typename IO, int D, bool VEC>
__device__ __forceinline__ void row_miss(const IO* upd, const IO* tgt, const IO* sub, int64_t row, double (&m)[D]) {
  IO u[D], t[D], s[D];
  load_row<IO, D, VEC>(upd + row * D, u);
  load_row<IO, D, VEC>(tgt + row * D, t);
  if (sub != nullptr) {      // wave-uniform
    load_row<IO, D, VEC>(sub + row * D, s);
#pragma unroll
    for (int c = 0; c < D; ++c) m[c] = (double)u[c] - ((double)t[c] - (double)s[c]);
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) m[c] = (double)u[c] - (double)t[c];
  }
}

template <int DOF, typename IO, int LPT, bool VEC>
__global__ void __launch_bounds__(64) loss_rows(const LossArgs a) {
  constexpr int D = 2 * DOF, TPW = 64 / LPT;
  const int lane = (int)threadIdx.x, l = lane % LPT;
  const int64_t b_raw = (int64_t)blockIdx.x * TPW + lane / LPT;
  const bool on = b_raw < a.B;
  const int64_t b = on ? b_raw : (int64_t)a.B - 1;
  const int n = a.n;
  const int64_t row0 = b * n;
  const IO *upd = (const IO*)a.update, *tgt = (const IO*)a.target, *sub = (const IO*)a.target_sub;
  double pos = 0.0, vel = 0.0;
  for (int i = l; i < n; i += LPT) {
    double m[D];
    row_miss<IO, D, VEC>(upd, tgt, sub, row0 + i, m);
#pragma unroll
    for (int c = 0; c < DOF; ++c) pos = pos + m[c] * m[c];
#pragma unroll
    for (int c = DOF; c < D; ++c) vel = vel + m[c] * m[c];
  }
  pos = group_sum<LPT>(pos);
  vel = group_sum<LPT>(vel);
  // columns 2, 3, 4: the three errors of the trajectory, converted (0 for an absent array)
  const IO* e = (const IO*)(l == 2 ? a.unw_gp : l == 3 ? a.unw_sg : l == 4 ? a.unw_obs : nullptr);
  double out = l == 0 ? pos : vel;
  if (l >= 2) out = e != nullptr ? (double)e[b] : 0.0;
  if (on && l < DGP_LOSS_PER_TRAJ) a.per_traj[b * DGP_LOSS_PER_TRAJ + l] = out;
}

__global__ void __launch_bounds__(kBatchLanes) loss_batch(const LossArgs a) {
  __shared__ double part[kBatchLanes / 64][DGP_LOSS_PER_TRAJ];
  const int t = (int)threadIdx.x;
  double s[DGP_LOSS_PER_TRAJ];
#pragma unroll
  for (int c = 0; c < DGP_LOSS_PER_TRAJ; ++c) s[c] = 0.0;
  int64_t b = t;
  for (; b + 3 * kBatchLanes < a.B; b += 4 * kBatchLanes) {      // four rows in flight per lane (one round of memory latency at B = 4096), added in row order
    double v[4][DGP_LOSS_PER_TRAJ];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int c = 0; c < DGP_LOSS_PER_TRAJ; ++c) v[k][c] = a.per_traj[(b + (int64_t)k * kBatchLanes) * DGP_LOSS_PER_TRAJ + c];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int c = 0; c < DGP_LOSS_PER_TRAJ; ++c) s[c] = s[c] + v[k][c];
    }
  }
  for (; b < a.B; b += kBatchLanes) {
#pragma unroll
    for (int c = 0; c < DGP_LOSS_PER_TRAJ; ++c) s[c] = s[c] + a.per_traj[b * DGP_LOSS_PER_TRAJ + c];
  }
#pragma unroll
  for (int c = 0; c < DGP_LOSS_PER_TRAJ; ++c) s[c] = group_sum<64>(s[c]);
  if ((t & 63) == 0) {
#pragma unroll
    for (int c = 0; c < DGP_LOSS_PER_TRAJ; ++c) part[t >> 6][c] = s[c];
  }
  __syncthreads();
  if (t != 0) return;
#pragma unroll
  for (int c = 0; c < DGP_LOSS_PER_TRAJ; ++c) {
    double v = part[0][c];
    for (int w = 1; w < kBatchLanes / 64; ++w) v = v + part[w][c];
    s[c] = v;
  }
  const double fb = (double)a.B, fbn = (double)a.B * (double)a.n;
  const double pos = s[0] / fbn, vel = s[1] / fbn, gp = s[2] / fb, sg = s[3] / fb, obs = s[4] / fb;
  const double ext = (gp + sg) + a.w.ext_obs_lambda * obs;
  const double total = (pos + a.w.vel_loss_lambda * vel) + a.w.ext_loss_weight * ext;
  a.terms[DGP_LOSS_TOTAL] = total;
  a.terms[DGP_LOSS_POS] = pos;
  a.terms[DGP_LOSS_VEL] = vel;
  a.terms[DGP_LOSS_COV] = 0.0;
  a.terms[DGP_LOSS_GP] = gp;
  a.terms[DGP_LOSS_SG] = sg;
  a.terms[DGP_LOSS_OBS] = obs;
  a.terms[DGP_LOSS_EXT] = ext;
}

template <int DOF, typename IO, bool VEC>
__global__ void __launch_bounds__(kBwdLanes) loss_backward(const LossBwdArgs a) {
  constexpr int D = 2 * DOF;
  const double g = a.g_total != nullptr ? *a.g_total : 1.0;
  const double fb = (double)a.B, fbn = (double)a.B * (double)a.n;
  const double c_ext = a.w.ext_loss_weight * g;
  const double k_pos = (2.0 * g) / fbn;
  const double k_vel = (2.0 * (a.w.vel_loss_lambda * g)) / fbn;
  const bool elems = a.g_update != nullptr || a.g_target != nullptr || a.g_target_sub != nullptr;      // wave-uniform
  const int64_t rows = elems ? (int64_t)a.B * a.n : (int64_t)a.B, stride = (int64_t)gridDim.x * kBwdLanes;
  const IO *upd = (const IO*)a.update, *tgt = (const IO*)a.target, *sub = (const IO*)a.target_sub;
  for (int64_t r = (int64_t)blockIdx.x * kBwdLanes + threadIdx.x; r < rows; r += stride) {
    if (elems) {
      double m[D];
      row_miss<IO, D, VEC>(upd, tgt, sub, r, m);
      IO gp_[D], gn_[D];
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const double v = m[c] * (c < DOF ? k_pos : k_vel);
        gp_[c] = (IO)v;
        gn_[c] = (IO)(-v);
      }
      if (a.g_update != nullptr) store_row<IO, D, VEC>((IO*)a.g_update + r * D, gp_);
      if (a.g_target != nullptr) store_row<IO, D, VEC>((IO*)a.g_target + r * D, gn_);
      if (a.g_target_sub != nullptr) store_row<IO, D, VEC>((IO*)a.g_target_sub + r * D, gp_);
    }
    if (r < a.B) {
      const IO ge = (IO)(c_ext / fb), go = (IO)((a.w.ext_obs_lambda * c_ext) / fb);
      if (a.g_unw_sg != nullptr) ((IO*)a.g_unw_sg)[r] = ge;
      if (a.g_unw_gp != nullptr) ((IO*)a.g_unw_gp)[r] = ge;
      if (a.g_unw_obs != nullptr) ((IO*)a.g_unw_obs)[r] = go;
    }
  }
}

// lanes per trajectory of loss_rows: from the number of states alone.  Its own thresholds (one state per lane up to 32 states), not dgp_group::lanes_for's: the
// butterfly order, and so the bits of per_traj, follow from them (tests/loss_oracle.py mirrors this rule).
int rows_lpt(int n) { return n <= 16 ? 16 : n <= 32 ? 32 : 64; }

bool aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }      // (null counts as aligned)

template <int DOF, typename IO, bool VEC>
hipError_t launch_rows(const LossArgs& a, hipStream_t s, const dgp_dev::Events& ev) {
  const int lpt = rows_lpt(a.n), tpw = 64 / lpt;
  const dim3 grid((unsigned)(((int64_t)a.B + tpw - 1) / tpw)), block(64);
  return dgp_dev::with_lpt(lpt, [&](auto L) { return dgp_dev::launch(loss_rows<DOF, IO, L, VEC>, grid, block, 0, s, ev, a); });
}

template <int DOF, typename IO>
hipError_t launch_forward(const LossArgs& a, hipStream_t s, const dgp_dev::Events& ev) {
  constexpr int VB = vec_bytes<IO, 2 * DOF>();
  const bool vec = aligned(a.update, VB) && aligned(a.target, VB) && aligned(a.target_sub, VB);
  const hipError_t e = vec ? launch_rows<DOF, IO, true>(a, s, ev) : launch_rows<DOF, IO, false>(a, s, ev);
  if (e != hipSuccess) return e;
  const dgp_dev::Events none = {nullptr, nullptr};
  return dgp_dev::launch(loss_batch, dim3(1), dim3(kBatchLanes), 0, s, none, a);
}

template <int DOF, typename IO>
hipError_t launch_backward(const LossBwdArgs& a, hipStream_t s, const dgp_dev::Events& ev) {
  constexpr int VB = vec_bytes<IO, 2 * DOF>();
  const bool vec = aligned(a.update, VB) && aligned(a.target, VB) && aligned(a.target_sub, VB) && aligned(a.g_update, VB) && aligned(a.g_target, VB) &&
                   aligned(a.g_target_sub, VB);
  const int64_t rows = (int64_t)a.B * a.n, want = (rows + kBwdLanes - 1) / kBwdLanes;
  const dim3 grid((unsigned)(want < kBwdMaxBlocks ? want : kBwdMaxBlocks)), block(kBwdLanes);
  if (vec) return dgp_dev::launch(loss_backward<DOF, IO, true>, grid, block, 0, s, ev, a);
  return dgp_dev::launch(loss_backward<DOF, IO, false>, grid, block, 0, s, ev, a);
}

int check_common(const char* who, int32_t dtype, int32_t batch, int32_t num_states, int32_t dof, const void* update, const void* target, const DgpLossWeights* w) {
  if (dtype != DGP_F32 && dtype != DGP_F64) return fail(DGP_EINVAL, "%s: dtype must be DGP_F32 or DGP_F64, got %d", who, dtype);
  if (batch < 1 || num_states < 1) return fail(DGP_EINVAL, "%s: batch and num_states must be positive, got %d and %d", who, batch, num_states);
  if (dof != 2 && dof != 3) return fail(DGP_EINVAL, "%s: dof must be 2 or 3, got %d", who, dof);
  if (!update || !target || !w) return fail(DGP_EINVAL, "%s: null update, target or weights", who);
  if (w->vel_loss_lambda != w->vel_loss_lambda || w->ext_obs_lambda != w->ext_obs_lambda || w->ext_loss_weight != w->ext_loss_weight)
    return fail(DGP_EINVAL, "%s: a weight (vel_loss_lambda, ext_obs_lambda, ext_loss_weight) is NaN", who);
  return DGP_OK;
}

}  // namespace

extern "C" int dgp_step_loss(int32_t dtype, int32_t batch, int32_t num_states, int32_t dof, const void* update, const void* target, const void* target_sub,
                             const void* unw_sg, const void* unw_gp, const void* unw_obs, const DgpLossWeights* w, double* terms, double* per_traj, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  const int rc = check_common("dgp_step_loss", dtype, batch, num_states, dof, update, target, w);
  if (rc != DGP_OK) return rc;
  if (!terms || !per_traj) return fail(DGP_EINVAL, "dgp_step_loss: null terms or per_traj (per_traj is the workspace of the batch sums)");
  LossArgs a;
  a.update = update; a.target = target; a.target_sub = target_sub;
  a.unw_sg = unw_sg; a.unw_gp = unw_gp; a.unw_obs = unw_obs;
  a.per_traj = per_traj; a.terms = terms; a.w = *w; a.B = batch; a.n = num_states;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = dgp_dev::with_dof_io(dof, dtype == DGP_F64, [&](auto DOF, auto io) { return launch_forward<DOF, decltype(io)>(a, s, ev); });
  return dgp_dev::hip_rc(e, "dgp_step_loss");
}

extern "C" int dgp_step_loss_backward(int32_t dtype, int32_t batch, int32_t num_states, int32_t dof, const void* update, const void* target,
                                      const void* target_sub, const DgpLossWeights* w, const double* g_total, void* g_update, void* g_target, void* g_target_sub,
                                      void* g_unw_sg, void* g_unw_gp, void* g_unw_obs, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  const int rc = check_common("dgp_step_loss_backward", dtype, batch, num_states, dof, update, target, w);
  if (rc != DGP_OK) return rc;
  if (!g_update && !g_target && !g_target_sub && !g_unw_sg && !g_unw_gp && !g_unw_obs) return fail(DGP_EINVAL, "dgp_step_loss_backward: every gradient output is null");
  LossBwdArgs a;
  a.update = update; a.target = target; a.target_sub = target_sub; a.g_total = g_total;
  a.g_update = g_update; a.g_target = g_target; a.g_target_sub = g_target_sub;
  a.g_unw_sg = g_unw_sg; a.g_unw_gp = g_unw_gp; a.g_unw_obs = g_unw_obs;
  a.w = *w; a.B = batch; a.n = num_states;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = dgp_dev::with_dof_io(dof, dtype == DGP_F64, [&](auto DOF, auto io) { return launch_backward<DOF, decltype(io)>(a, s, ev); });
  return dgp_dev::hip_rc(e, "dgp_step_loss_backward");
}
