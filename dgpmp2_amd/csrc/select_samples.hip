// select_samples.hip -- dgp_select_samples: the back half of a multi-start in ONE launch (gfx950 / CDNA4): the dense collision check of every optimised sample of
// every problem, the total order of a problem's samples, and the chosen trajectory gathered into th_best.
//
// What it builds: nothing the reference has -- it optimises one trajectory per problem.  The front half is dgp_prior_samples (S initial trajectories per problem) and
// dgp_gn_solve over the B S rows; this unit decides, per problem, which optimised sample to keep.  include/dgpmp2_hip.h states the rule (status bits, tiers, the
// total order), tests/select_oracle.py restates it, and the kernel is held against that exactly: every key of the order is an input or a bit-exact intermediate.
//
// Mapping: one workgroup per problem.  A sample occupies a group of LPT = 16 / 32 / 64 lanes (dgp_group::lanes_for(N_d), as dgp_gp_interpolate), 64 / LPT samples per
// wavefront, up to kMaxWaves wavefronts; more samples than the workgroup has groups are walked in passes.  The dense check of a sample is dgp_dense_walk.h's -- the
// walk and the butterflies gp_interpolate.hip runs, so sample_summary is dgp_gp_interpolate's summary bit for bit.  Lane 0 of a group parks (tier, max penetration,
// score, status) of its sample in LDS (24 bytes per sample, sized by the launch); after one barrier thread s counts the samples that precede sample s -- its rank, a
// pure function of the keys: no sort network, S compares per sample -- and stores order / status; the thread of rank 0 stores best and the problem summary.  After
// a second barrier the whole workgroup copies row `best` to th_best as 16- / 8- / 4-byte words, whichever the two addresses and the row size allow: the same bits
// either way, no arithmetic.  Lane groups past S recompute the last sample and store nothing (no divergent shuffles).  No atomics, nothing allocated or
// synchronised on the host side.
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

constexpr int kMaxWaves = 16;       // wavefronts of a workgroup
constexpr int kMaxSamples = 1024;   // 24 KB of keys in LDS

struct SelectShape { int lpt, waves, passes; };
inline SelectShape select_shape(int nd, int num_samples) {
  SelectShape sh;
  sh.lpt = dgp_group::lanes_for(nd);
  const int tpw = 64 / sh.lpt;
  const int need = (num_samples + tpw - 1) / tpw;
  sh.waves = need < kMaxWaves ? need : kMaxWaves;
  sh.passes = (num_samples + sh.waves * tpw - 1) / (sh.waves * tpw);
  return sh;
}

struct SelectArgs {
  dgp::GnParams p;             // B problems, n, th, the grid and the constants of the bilinear lookup (dgp_host::fill_call); dt
  const void* score;           // io_dtype or null
  const int32_t* exclude;      // or null
  const int32_t* env_index;    // (B) or null
  void* th_best;               // (B, n, d) or null
  int32_t* best;               // (B) or null
  int32_t* order;              // (B, S) or null
  int32_t* status;             // (B, S) or null
  double* sample_summary;      // (B, S, DGP_DENSE_COUNT) or null
  double* problem_summary;     // (B, DGP_SELECT_COUNT) or null
  double eps;
  dgp_dense::Limits lim;
  int32_t k1, nd;              // num_inter + 1, N_d
  int32_t S, sample_major, require_inside;
};
static_assert(sizeof(SelectArgs) <= 4096, "kernel-argument segment");

// does the sample with keys (ta, ma, sa, ia) precede the one with (tb, mb, sb, ib)?  The header's total order.
__device__ __forceinline__ bool precedes(int ta, double ma, double sa, int ia, int tb, double mb, double sb, int ib) {
  if (ta != tb) return ta < tb;
  if (ta == 1) {
    if (ma < mb) return true;
    if (mb < ma) return false;
  }
  if (ta < 2) {
    if (sa < sb) return true;
    if (sb < sa) return false;
  }
  return ia < ib;
}

template <typename W>
__device__ __forceinline__ void copy_words(const void* src, void* dst, int64_t bytes, int tid, int nthreads) {
  const W* s = (const W*)src;
  W* d = (W*)dst;
  const int64_t count = bytes / (int64_t)sizeof(W);
  for (int64_t k = tid; k < count; k += nthreads) d[k] = s[k];
}

template <int DOF, typename IO, int LPT>
__global__ void __launch_bounds__(64 * kMaxWaves) select_samples_kernel(const SelectArgs a) {
  constexpr int D = 2 * DOF, TPW = 64 / LPT;
  extern __shared__ double lds[];
  const dgp::GnParams& p = a.p;
  const int S = a.S;
  double* k_pen = lds;                       // [S]
  double* k_score = lds + S;                 // [S]
  int* k_tier = (int*)(lds + 2 * (int64_t)S);      // [S]
  int* k_status = k_tier + S;                // [S]
  __shared__ int s_best;

  const int tid = (int)threadIdx.x, nthreads = (int)blockDim.x;
  const int lane = tid & 63, l = lane % LPT, gbase = lane - l;
  const int groups = (nthreads / 64) * TPW;      // samples per pass
  const int64_t b = (int64_t)blockIdx.x;
  const int n = p.n, k1 = a.k1, nd = a.nd;
  const int64_t B = (int64_t)p.B;
  const bool look = p.sdf != nullptr;            // uniform
  const int64_t env = a.env_index != nullptr ? (int64_t)a.env_index[b] : b;
  const IO* grid = look ? (const IO*)p.sdf + env * p.sdf_bstride : nullptr;
  const uint64_t gmask = (~0ull >> (64 - LPT)) << gbase;

  for (int s0 = 0; s0 < S; s0 += groups) {       // uniform trip count
    const int s_raw = s0 + (tid / 64) * TPW + lane / LPT;
    const bool on = s_raw < S;
    const int s = on ? s_raw : S - 1;
    const int64_t row = a.sample_major ? (int64_t)s * B + b : b * S + s;      // of th, score and exclude
    const IO* th = (const IO*)p.th + row * n * D;
    dgp_dense::Partials r;
    dgp_dense::Flags f = {false, false};
    dgp_dense::walk<DOF, IO, LPT, true>(p, th, grid, (IO*)nullptr, (IO*)nullptr, look, a.eps, k1, nd, l, r, a.lim, f);
    dgp_dense::reduce<LPT>(r);
    const bool any_out = (__ballot(f.outside) & gmask) != 0ull, any_nf = (__ballot(f.nonfinite) & gmask) != 0ull;
    if (a.sample_summary != nullptr && on && l < DGP_DENSE_COUNT)
      a.sample_summary[(b * S + s) * DGP_DENSE_COUNT + l] = dgp_dense::summary_column(l, r, nd);
    if (on && l == 0) {
      const double sc = a.score != nullptr ? (double)((const IO*)a.score)[row] : 0.0;
      const double pen = look ? r.m_pen : 0.0;
      const bool excluded = a.exclude != nullptr && a.exclude[row] != 0;
      const bool colliding = look && r.cnt != 0;
      const bool nonfinite = any_nf || !(sc - sc == 0.0) || pen != pen;
      const int st = (colliding ? DGP_SEL_COLLIDING : 0) | (any_out ? DGP_SEL_OUTSIDE : 0) | (nonfinite ? DGP_SEL_NON_FINITE : 0) | (excluded ? DGP_SEL_EXCLUDED : 0);
      const int tier = (nonfinite || excluded) ? 2 : ((colliding || (a.require_inside != 0 && any_out)) ? 1 : 0);
      k_pen[s] = pen; k_score[s] = sc; k_tier[s] = tier; k_status[s] = st;
    }
  }
  __syncthreads();

  for (int s = tid; s < S; s += nthreads) {
    const int ts = k_tier[s], st = k_status[s];
    const double ms = k_pen[s], ss = k_score[s];
    int rank = 0, accepted = 0;
    for (int u = 0; u < S; ++u) {              // every thread reads the same entry: LDS broadcasts
      const int tu = k_tier[u];
      rank += precedes(tu, k_pen[u], k_score[u], u, ts, ms, ss, s) ? 1 : 0;
      accepted += tu == 0 ? 1 : 0;
    }
    if (a.order != nullptr) a.order[b * S + rank] = s;
    if (a.status != nullptr) a.status[b * S + s] = st;
    if (rank == 0) {
      s_best = s;
      if (a.best != nullptr) a.best[b] = s;
      if (a.problem_summary != nullptr) {
        double* ps = a.problem_summary + b * DGP_SELECT_COUNT;
        ps[DGP_SELECT_SOLVED] = ts == 0 ? 1.0 : 0.0;
        ps[DGP_SELECT_NUM_ACCEPTED] = (double)accepted;
        ps[DGP_SELECT_BEST_INDEX] = (double)s;
        ps[DGP_SELECT_BEST_SCORE] = ss;
        ps[DGP_SELECT_BEST_MAX_PENETRATION] = ms;
        ps[DGP_SELECT_BEST_STATUS] = (double)st;
      }
    }
  }
  if (a.th_best == nullptr) return;            // uniform
  __syncthreads();
  const int sb = s_best;
  const int64_t row = a.sample_major ? (int64_t)sb * B + b : b * S + sb;
  const int64_t bytes = (int64_t)n * D * (int64_t)sizeof(IO);
  const char* src = (const char*)p.th + row * bytes;
  char* dst = (char*)a.th_best + b * bytes;
  const uintptr_t mis = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)bytes;      // uniform
  if ((mis & 15u) == 0) copy_words<uint4>(src, dst, bytes, tid, nthreads);
  else if ((mis & 7u) == 0) copy_words<uint2>(src, dst, bytes, tid, nthreads);
  else copy_words<uint32_t>(src, dst, bytes, tid, nthreads);      // (fp32 rows off an 8-byte boundary; a row is a whole number of 8-byte pairs)
}

}  // namespace

extern "C" int dgp_select_samples(const DgpHandle* h, int32_t batch, int32_t num_samples, const void* th, const void* score, const int32_t* exclude, const DgpSdf* sdf,
                                  const int32_t* env_index, const DgpSelectParams* sp, void* th_best, int32_t* best, int32_t* order, int32_t* status,
                                  double* sample_summary, double* problem_summary, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  if (!h) return fail(DGP_EINVAL, "dgp_select_samples: null handle (h)");
  if (!th) return fail(DGP_EINVAL, "dgp_select_samples: th must be a non-null device pointer");
  if (!sp) return fail(DGP_EINVAL, "dgp_select_samples: p (DgpSelectParams) must be non-null");
  if (sp->struct_size != sizeof(DgpSelectParams))
    return fail(DGP_EINVAL, "dgp_select_samples: DgpSelectParams struct_size mismatch: caller %u, library %zu", sp->struct_size, sizeof(DgpSelectParams));
  if (batch < 1) return fail(DGP_EINVAL, "dgp_select_samples: batch must be positive, got %d", batch);
  if (num_samples < 1 || num_samples > kMaxSamples)
    return fail(DGP_EINVAL, "dgp_select_samples: num_samples must be in 1..%d (the keys of a problem's samples stay in LDS), got %d", kMaxSamples, num_samples);
  if ((int64_t)batch * num_samples > (int64_t)0x7fffffff)
    return fail(DGP_EINVAL, "dgp_select_samples: batch * num_samples = %lld trajectories exceed one launch (2^31 - 1)", (long long)batch * num_samples);
  if (sp->num_inter < 0 || sp->num_inter > dgp_host::kMaxNumInter)
    return fail(DGP_EINVAL, "dgp_select_samples: num_inter must be in 0..%d, got %d", dgp_host::kMaxNumInter, sp->num_inter);
  if (!(sp->eps - sp->eps == 0.0)) return fail(DGP_EINVAL, "dgp_select_samples: eps must be finite, got %g", sp->eps);
  if (!th_best && !best && !order && !status && !sample_summary && !problem_summary)
    return fail(DGP_EINVAL, "dgp_select_samples: th_best, best, order, status, sample_summary and problem_summary are all null");
  const bool has_sdf = sdf && sdf->data;
  if (sample_summary && !has_sdf) return fail(DGP_EINVAL, "dgp_select_samples: sample_summary needs the signed-distance grid (sdf)");
  if (env_index && !has_sdf) return fail(DGP_EINVAL, "dgp_select_samples: env_index needs the signed-distance grid (sdf)");
  SelectArgs a;
  const int rc = dgp_host::fill_call(h, batch, th, /*start=*/th, /*goal=*/th, sdf, nullptr, a.p, /*sdf_optional=*/true);      // (no start / goal here: th stands in for the null checks)
  if (rc != DGP_OK) return rc;
  a.k1 = sp->num_inter + 1;
  a.nd = dgp_host::dense_states(a.p.n, sp->num_inter);
  if (has_sdf && a.nd < 3)
    return fail(DGP_EINVAL, "dgp_select_samples: the collision check (sdf) needs at least 3 dense states (no interior state), got %d: raise num_inter", a.nd);
  a.score = score; a.exclude = exclude; a.env_index = env_index;
  a.th_best = th_best; a.best = best; a.order = order; a.status = status; a.sample_summary = sample_summary; a.problem_summary = problem_summary;
  a.eps = sp->eps;
  a.lim = dgp_dense::Limits{h->cfg.x_lims[0], h->cfg.x_lims[1], h->cfg.y_lims[0], h->cfg.y_lims[1]};
  a.S = num_samples; a.sample_major = sp->sample_major != 0 ? 1 : 0; a.require_inside = sp->require_inside != 0 ? 1 : 0;
  const SelectShape sh = select_shape(a.nd, num_samples);
  const dim3 grid((unsigned)a.p.B), block((unsigned)(64 * sh.waves));
  const unsigned lds = (unsigned)(a.S * (2 * sizeof(double) + 2 * sizeof(int)));
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = dgp_dev::with_dof_io(h->cfg.dof, h->cfg.io_dtype == DGP_F64, [&](auto dof, auto io) {
    return dgp_dev::with_lpt(sh.lpt, [&](auto L) { return dgp_dev::launch(select_samples_kernel<dof, decltype(io), L>, grid, block, lds, s, ev, a); });
  });
  return dgp_dev::hip_rc(e, "dgp_select_samples");
}

extern "C" int dgp_select_launch_shape(const DgpHandle* h, int32_t num_samples, int32_t num_inter, int32_t* lanes_per_traj, int32_t* waves_per_group, int32_t* passes) {
  if (!h) return fail(DGP_EINVAL, "dgp_select_launch_shape: null handle (h)");
  if (num_samples < 1 || num_samples > kMaxSamples) return fail(DGP_EINVAL, "dgp_select_launch_shape: num_samples must be in 1..%d, got %d", kMaxSamples, num_samples);
  if (num_inter < 0 || num_inter > dgp_host::kMaxNumInter) return fail(DGP_EINVAL, "dgp_select_launch_shape: num_inter must be in 0..%d, got %d", dgp_host::kMaxNumInter, num_inter);
  const SelectShape sh = select_shape(dgp_host::dense_states(h->cfg.num_states, num_inter), num_samples);
  if (lanes_per_traj) *lanes_per_traj = sh.lpt;
  if (waves_per_group) *waves_per_group = sh.waves;
  if (passes) *passes = sh.passes;
  return DGP_OK;
}
