// heading_lift.hip -- dgp_heading_lift: planar trajectories (B,n,4) lifted to problems of the non-holonomic x-y-heading robot -- start, goal (B,1,6) and th (B,n,6) --
// in ONE launch (gfx950 / CDNA4).  The heading follows the path's tangent continuously (the sum of the signed turns between consecutive tangents: unwrapped by
// construction) and is blended into the end headings; the velocities are the path's own central differences.  The reference's rule -- a heading linear in time and one
// constant velocity (straight_line_trajb, utils/planner_utils.py:47-56) -- is DGP_HEADING_LINEAR / DGP_VEL_KEEP.  include/dgpmp2_hip.h states the rule and its fp64
// operation order, tests/heading_oracle.py restates it, and the kernel is held against that bit for bit (the atan2 of generated turns apart: turns_out / turns_in).
//
// Mapping (prior_samples.hip's): one trajectory per group of LPT = 16 / 32 / 64 lanes (dgp_prior::launch_shape(n)), lane l holds state l.  Neighbour positions and
// headings come through __shfl_up / __shfl_down; the forward fill of degenerate tangents is an inclusive max-scan of the last valid index and one indexed shuffle;
// psi is the additive Hillis-Steele scan of the header's SCAN.  Past 64 states (LONG) a wavefront walks blocks of 64 states, carrying the last state's position, filled
// tangent, psi and heading; the state behind a block's last lane (its position, its turn and so its heading) is formed by that lane alone from two extra loads.  LONG
// runs the blocks twice: the goal blend needs psi_N, and the turn of row 0 the first valid tangent, before any row can be stored.
// A row whose filled tangent is the LEADING fill (no valid tangent at or before the row in front of it) has turn atan2(+0, |u|^2) = +0.0 whatever u is: the kernel
// writes that zero without knowing the first valid tangent, which only turn_0 needs.
// Traffic: B n 10 elements (4 read, 6 written) plus the optional arrays; rows move as 8- / 16-byte vectors where the pointers allow.  No atomics, nothing allocated or
// synchronised.  Lane groups past the end of a ragged launch recompute the last trajectory and store nothing (no divergent shuffles).
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

constexpr double kPi = 3.141592653589793, kTwoPi = 6.283185307179586;
constexpr uint32_t kHeadingStream = 2u;      // counter word 3: dgp_sample_problems uses 0 and 1

struct LiftArgs {
  const void* th2;                              // (B,n,4)
  const double *start_heading, *goal_heading;   // (B) or null
  const double* turns_in;                       // (B,n) or null
  void *start, *goal, *th;                      // (B,1,6), (B,1,6), (B,n,6)
  double* turns_out;                            // (B,n) or null
  int32_t* info;                                // (B) or null
  int64_t B;
  int32_t n, heading_mode, start_end, goal_end, velocity_mode, blend;
  uint64_t first_problem;
  uint32_t key0, key1;
  double total_time, delta;                     // total_time_sec, total_time_sec / N
  int32_t vec_in, vec_out;                      // th2 / th allow the vector accesses of load_row / store_row
};

using dgp_group::group_scan;
using dgp_rowio::load_row;
using dgp_rowio::store_row;

template <int LPT>
__device__ __forceinline__ int group_max_scan(int x, int l) {
#pragma unroll
  for (int off = 1; off < LPT; off <<= 1) {
    const int lo = __shfl_up(x, off, LPT);
    x = (l >= off && lo > x) ? lo : x;
  }
  return x;
}

__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }
__device__ __forceinline__ bool degenerate(double tx, double ty) { return (tx == 0.0 && ty == 0.0) || !finite(tx) || !finite(ty); }
__device__ __forceinline__ double wrap(double a) { return a - kTwoPi * rint(a / kTwoPi); }

// the arguments of the atan2 of turn_i, i >= 1: (cross, dot) of the filled tangents of rows i - 1 and i; (+0, 1) where row i - 1 holds the leading fill
__device__ __forceinline__ void turn_args(bool prev_has, double upx, double upy, double ux, double uy, double& c, double& d) {
  c = upx * uy - upy * ux;
  c = c == 0.0 ? 0.0 : c;
  d = upx * ux + upy * uy;
  if (!prev_has) { c = 0.0; d = 1.0; }
}

// what every row of a trajectory shares once turn_0 and psi_N are known
struct Blend {
  bool tangent;
  int N;
  double ths, thg;         // the end headings
  double e_s, e_g, base;   // TANGENT
  double th0, thN;         // TANGENT: the headings rows 0 and N store
  double blend;
};

__device__ __forceinline__ double heading(const Blend& k, int i, double psi) {
  if (k.tangent) {
    const double phi = k.base + psi;
    const double ws = fmax(0.0, 1.0 - (double)i / k.blend), wg = fmax(0.0, 1.0 - (double)(k.N - i) / k.blend);
    double th = (phi + ws * k.e_s) + wg * k.e_g;
    if (i == 0) th = k.th0;
    if (i == k.N) th = k.thN;
    return th;
  }
  return k.ths * (double)(k.N - i) * 1.0 / (double)k.N * 1.0 + k.thg * (double)i * 1.0 / (double)k.N * 1.0;
}

template <typename IO, int LPT, bool LONG>
__global__ void __launch_bounds__(64) heading_lift_kernel(const LiftArgs a) {
  constexpr int TPW = 64 / LPT;
  static_assert(!LONG || LPT == 64, "blocks of 64 states");
  const int lane = (int)threadIdx.x, l = lane % LPT, gbase = lane - l;
  const int64_t b_raw = (int64_t)blockIdx.x * TPW + lane / LPT;
  const bool on = b_raw < a.B;
  const int64_t b = on ? b_raw : a.B - 1;
  const int n = a.n, N = n - 1;
  const IO* src = (const IO*)a.th2 + b * (int64_t)n * 4;
  IO* dst = (IO*)a.th + b * (int64_t)n * 6;
  const double* tin = a.turns_in != nullptr ? a.turns_in + b * (int64_t)n : nullptr;
  const bool tangent = a.heading_mode == DGP_HEADING_TANGENT, diff = a.velocity_mode == DGP_VEL_DIFF;

  // the end headings
  Blend k;
  k.tangent = tangent; k.N = N; k.blend = (double)a.blend;
  k.ths = k.thg = 0.0; k.e_s = k.e_g = k.base = k.th0 = k.thN = 0.0;
  bool f_nonfinite = false;
  if (a.start_end == DGP_END_RANDOM || a.goal_end == DGP_END_RANDOM) {
    const uint64_t problem = a.first_problem + (uint64_t)b;
    uint32_t w[4];
    dgp::philox4x32_10((uint32_t)problem, (uint32_t)(problem >> 32), 0u, kHeadingStream, a.key0, a.key1, w);
    const double u0 = (double)((((uint64_t)w[0] << 32) | w[1]) >> 11) * 0x1.0p-53;
    const double u1 = (double)((((uint64_t)w[2] << 32) | w[3]) >> 11) * 0x1.0p-53;
    if (a.start_end == DGP_END_RANDOM) k.ths = (-kPi) + u0 * kTwoPi;
    if (a.goal_end == DGP_END_RANDOM) k.thg = (-kPi) + u1 * kTwoPi;
  }
  if (a.start_end == DGP_END_SUPPLIED) { k.ths = a.start_heading[b]; f_nonfinite = f_nonfinite || !finite(k.ths); }
  if (a.goal_end == DGP_END_SUPPLIED) { k.thg = a.goal_heading[b]; f_nonfinite = f_nonfinite || !finite(k.thg); }

  const int last_k0 = LONG ? (N / 64) * 64 : 0, last_l = N - last_k0;      // the block and the lane of state N (not LONG: n <= LPT, block 0)
  double Fx = 1.0, Fy = 0.0;      // the first non-degenerate tangent, (1, 0) if there is none
  bool any_valid = false;
  double psiN = 0.0, turn0 = 0.0;
  bool f_filled = false, f_big = false;
  // LONG: pass 0 finds the first valid tangent and psi_N; pass 1 runs the blocks again and stores.  Otherwise the one block does both in one trip.
  constexpr int FIRST = LONG ? 0 : 1;
  for (int pass = FIRST; pass < 2; ++pass) {
    double c_x = 0.0, c_y = 0.0, c_ux = 0.0, c_uy = 0.0, c_psi = 0.0, c_th = 0.0;      // state k0 - 1: position, filled tangent, psi, heading
    int c_has = 0;                                                                    // ... a valid tangent at or before it
    for (int k0 = 0; k0 <= last_k0; k0 += LPT) {
      const int st = k0 + l, sr = st <= N ? st : N;      // (lanes past the last state: row N again; their values reach no stored state)
      const bool live = st <= N;
      IO q[4];
      load_row<IO, 4>(src + (int64_t)sr * 4, q, a.vec_in != 0);
      const double x = (double)q[0], y = (double)q[1];
      // t_i = p_hi - p_lo, lo = max(i - 1, 0), hi = min(i + 1, N)
      double xp = __shfl_up(x, 1, LPT), yp = __shfl_up(y, 1, LPT);
      if (l == 0) { xp = k0 > 0 ? c_x : x; yp = k0 > 0 ? c_y : y; }
      double xn = __shfl_down(x, 1, LPT), yn = __shfl_down(y, 1, LPT);
      if (st >= N) { xn = x; yn = y; }
      else if (LONG && l == 63) { xn = (double)src[(int64_t)(st + 1) * 4]; yn = (double)src[(int64_t)(st + 1) * 4 + 1]; }
      const double tx = xn - xp, ty = yn - yp;
      const int span = (sr < N ? sr + 1 : N) - (sr > 0 ? sr - 1 : 0);
      const bool deg = degenerate(tx, ty);

      double turn = 0.0, psi = 0.0, ux = 0.0, uy = 0.0;
      int has = 0;
      if (tangent) {      // (uniform over the launch)
        // forward fill: the last valid index at or before each lane, then that lane's tangent; none in this block: the carried one
        const int v = group_max_scan<LPT>((!deg && live) ? l : -1, l);
        ux = __shfl(tx, gbase + (v > 0 ? v : 0)); uy = __shfl(ty, gbase + (v > 0 ? v : 0));
        has = v >= 0 ? 1 : c_has;
        if (v < 0) { ux = c_ux; uy = c_uy; }
        // the first valid tangent of the trajectory
        const uint64_t gmask = (~0ull >> (64 - LPT)) << gbase;
        const uint64_t valid = __ballot(!deg && live) & gmask;
        const int f = valid != 0ull ? __ffsll((unsigned long long)valid) - 1 : lane;
        const double fx = __shfl(tx, f), fy = __shfl(ty, f);
        if (!any_valid && valid != 0ull) { Fx = fx; Fy = fy; any_valid = true; }
        double upx = __shfl_up(ux, 1, LPT), upy = __shfl_up(uy, 1, LPT);
        int phas = __shfl_up(has, 1, LPT);
        if (l == 0) { upx = c_ux; upy = c_uy; phas = c_has; }
        if (tin != nullptr) turn = tin[sr];
        else {
          double c, d;
          turn_args(phas != 0, upx, upy, ux, uy, c, d);
          if (st == 0) { c = Fy; d = Fx; }      // turn_0 (LONG: F is complete in pass 1, and pass 0 does not read this lane's turn)
          turn = atan2(c, d);
        }
        psi = group_scan<LPT>(st == 0 ? 0.0 : turn, l);
        if (k0 > 0) psi = c_psi + psi;
        if (k0 == 0) turn0 = __shfl(turn, gbase);
        if (pass == FIRST && k0 == last_k0) psiN = __shfl(psi, gbase + last_l);
      }
      if (LONG && pass == 0) {
        c_x = __shfl(x, 63); c_y = __shfl(y, 63); c_ux = __shfl(ux, 63); c_uy = __shfl(uy, 63); c_has = __shfl(has, 63); c_psi = __shfl(psi, 63);
        continue;
      }
      if (tangent && (!LONG || k0 == 0)) {      // LONG: once per trajectory -- turn_0 is block 0's and psi_N pass 0's, so later blocks would only form the same values again
        k.e_s = a.start_end == DGP_END_TANGENT ? 0.0 : wrap(k.ths - turn0);
        k.th0 = a.start_end == DGP_END_TANGENT ? turn0 : k.ths;
        k.base = k.th0 - k.e_s;
        const double phiN = k.base + psiN;
        k.e_g = a.goal_end == DGP_END_TANGENT ? 0.0 : wrap(k.thg - phiN);
        k.thN = phiN + k.e_g;
      }
      const double th = heading(k, sr, psi);
      double thp = __shfl_up(th, 1, LPT);
      if (l == 0) thp = k0 > 0 ? c_th : th;
      double thn = __shfl_down(th, 1, LPT);
      if (st >= N) thn = th;
      else if (LONG && l == 63 && diff) {
        // state j = st + 1 opens the next block: psi_j = psi_st + turn_j by the SCAN's own rule (the block's first index takes no partner), turn_j from t_j
        const int j = st + 1;
        double psj = 0.0;
        if (tangent) {
          double tj;
          if (tin != nullptr) tj = tin[j];
          else {
            const int jh = j < N ? j + 1 : N;
            const double tjx = (double)src[(int64_t)jh * 4] - x, tjy = (double)src[(int64_t)jh * 4 + 1] - y;
            const bool dj = degenerate(tjx, tjy);
            double c, d;
            turn_args(has != 0, ux, uy, dj ? ux : tjx, dj ? uy : tjy, c, d);
            tj = atan2(c, d);
          }
          psj = psi + tj;
        }
        thn = heading(k, j, psj);
      }
      const double den = (double)span * a.delta;
      IO o[6];
      o[0] = q[0]; o[1] = q[1]; o[2] = (IO)th;
      if (diff) { o[3] = (IO)(tx / den); o[4] = (IO)(ty / den); o[5] = (IO)((thn - thp) / den); }
      else {
        const double w0 = tangent ? k.th0 : k.ths, wN = tangent ? k.thN : k.thg;
        o[3] = q[2]; o[4] = q[3]; o[5] = (IO)((wN - w0) / a.total_time * 1.0);
      }
      if (live) {
        if (on) {
          store_row<IO, 6>(dst + (int64_t)st * 6, o, a.vec_out != 0);
          if (a.turns_out != nullptr) a.turns_out[b * (int64_t)n + st] = turn;
          if (st == 0 || st == N) {
            IO* e = (IO*)(st == 0 ? a.start : a.goal) + b * 6;
            e[0] = o[0]; e[1] = o[1]; e[2] = o[2]; e[3] = (IO)0.0; e[4] = (IO)0.0; e[5] = (IO)0.0;
          }
        }
        f_filled = f_filled || (tangent && deg);
        f_big = f_big || (tangent && st >= 1 && fabs(turn) > kPi / 2.0);
        f_nonfinite = f_nonfinite || !finite(x) || !finite(y);
      }
      if constexpr (LONG) {
        c_x = __shfl(x, 63); c_y = __shfl(y, 63); c_ux = __shfl(ux, 63); c_uy = __shfl(uy, 63); c_has = __shfl(has, 63); c_psi = __shfl(psi, 63);
        c_th = __shfl(th, 63);
      }
    }
  }
  const uint64_t gmask = (~0ull >> (64 - LPT)) << gbase;
  const bool any_filled = (__ballot(f_filled) & gmask) != 0ull, any_big = (__ballot(f_big) & gmask) != 0ull, any_nf = (__ballot(f_nonfinite) & gmask) != 0ull;
  if (a.info != nullptr && on && l == 0) a.info[b] = ((tangent && !any_valid) ? 1 : 0) | (any_filled ? 2 : 0) | (any_big ? 4 : 0) | (any_nf ? 8 : 0);
}

template <typename IO>
hipError_t launch_n(const LiftArgs& a, hipStream_t s, const dgp_dev::Events& ev) {
  const dgp_prior::LaunchShape sh = dgp_prior::launch_shape(a.n);
  const int tpw = 64 / sh.lpt;
  const dim3 grid((unsigned)((a.B + tpw - 1) / tpw)), block(64);
  if (sh.blocks > 1) return dgp_dev::launch(heading_lift_kernel<IO, 64, true>, grid, block, 0, s, ev, a);
  return dgp_dev::with_lpt(sh.lpt, [&](auto L) { return dgp_dev::launch(heading_lift_kernel<IO, L, false>, grid, block, 0, s, ev, a); });
}

}  // namespace

extern "C" int dgp_heading_lift(const DgpHandle* h, int32_t batch, const DgpHeadingParams* p, const void* th2, const double* start_heading, const double* goal_heading,
                                const double* turns_in, void* start, void* goal, void* th, double* turns_out, int32_t* info, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  if (!h) return fail(DGP_EINVAL, "null handle");
  const DgpConfig& c = *reinterpret_cast<const DgpConfig*>(h);      // DgpHandle's first member (dgp_host.h holds that with a static_assert); this unit needs nothing else of it
  if (!p || !th2 || !start || !goal || !th) return fail(DGP_EINVAL, "dgp_heading_lift: params, th2, start, goal and th must be non-null");
  if (c.dof != 3) return fail(DGP_EINVAL, "dgp_heading_lift: the handle must be one of the x-y-heading robot (dof 3), got dof %d", c.dof);
  if (batch < 1) return fail(DGP_EINVAL, "dgp_heading_lift: batch must be positive, got %d", batch);
  if (p->heading_mode != DGP_HEADING_LINEAR && p->heading_mode != DGP_HEADING_TANGENT) return fail(DGP_EINVAL, "dgp_heading_lift: unknown heading_mode %d", p->heading_mode);
  if (p->velocity_mode != DGP_VEL_KEEP && p->velocity_mode != DGP_VEL_DIFF) return fail(DGP_EINVAL, "dgp_heading_lift: unknown velocity_mode %d", p->velocity_mode);
  const int32_t ends[2] = {p->start_end, p->goal_end};
  for (int e = 0; e < 2; ++e) {
    if (ends[e] != DGP_END_SUPPLIED && ends[e] != DGP_END_TANGENT && ends[e] != DGP_END_RANDOM)
      return fail(DGP_EINVAL, "dgp_heading_lift: unknown %s %d", e ? "goal_end" : "start_end", ends[e]);
    if (ends[e] == DGP_END_TANGENT && p->heading_mode == DGP_HEADING_LINEAR)
      return fail(DGP_EINVAL, "dgp_heading_lift: DGP_END_TANGENT needs DGP_HEADING_TANGENT (the linear rule forms no tangent)");
    if (ends[e] == DGP_END_SUPPLIED && !(e ? goal_heading : start_heading))
      return fail(DGP_EINVAL, "dgp_heading_lift: DGP_END_SUPPLIED needs the %s array", e ? "goal_heading" : "start_heading");
  }
  const int32_t N = c.num_states - 1;
  if (p->blend < 1 || p->blend > N) return fail(DGP_EINVAL, "dgp_heading_lift: blend must be in 1..%d (num_states - 1), got %d", N, p->blend);
  LiftArgs a;
  a.th2 = th2; a.start_heading = start_heading; a.goal_heading = goal_heading; a.turns_in = turns_in;
  a.start = start; a.goal = goal; a.th = th; a.turns_out = turns_out; a.info = info;
  a.B = batch; a.n = c.num_states;
  a.heading_mode = p->heading_mode; a.start_end = p->start_end; a.goal_end = p->goal_end; a.velocity_mode = p->velocity_mode; a.blend = p->blend;
  a.first_problem = p->first_problem;
  a.key0 = (uint32_t)(p->seed & 0xffffffffu); a.key1 = (uint32_t)(p->seed >> 32);
  a.total_time = c.total_time_sec;
  a.delta = c.total_time_sec / (double)N;
  const bool f64 = c.io_dtype == DGP_F64;
  a.vec_in = (reinterpret_cast<uintptr_t>(th2) & 15u) == 0 ? 1 : 0;                       // rows of 16 / 32 bytes as 16-byte vectors
  a.vec_out = (reinterpret_cast<uintptr_t>(th) & (f64 ? 15u : 7u)) == 0 ? 1 : 0;          // rows of 48 bytes as 16-byte vectors, the 24-byte rows of fp32 as 8-byte ones
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = f64 ? launch_n<double>(a, s, ev) : launch_n<float>(a, s, ev);
  return dgp_dev::hip_rc(e, "dgp_heading_lift");
}
