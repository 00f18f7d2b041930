// init_paths.hip -- dgp_init_paths: a collision-free initial trajectory from the start to the goal for every problem of a batch, ONE launch (gfx950 / CDNA4).
//
// What it stands in for: the reference's --rrt_star_init (datasets/generate_optimal_paths_gpmp2.py:95-110, :156-159; generate_2d_dataset.py:225-226): an OMPL RRT* run
// of 4 seconds per problem, interpolate(num_states) and path_to_traj_avg_vel (utils/planner_utils.py:60-71).  RRT* is randomised and OMPL is not part of this build:
// the PATH has no counterpart in the reference and no fixture from it.  What has one: the validity rule -- RRTStar.isStateValid -> Env2D.is_feasible(state,
// sphere_radius + epsilon_dist) (diff_gpmp2/ompl_rrtstar.py:18, :48-50), here "a cell is free where its stored distance > clearance" -- and the velocities of
// path_to_traj_avg_vel.  The path is the 5-7 (axis / diagonal) shortest grid path to the goal, traced greedily through its cost-to-go field; include/dgpmp2_hip.h
// states the rule, tests/paths_oracle.py restates it, and the kernel is held against that bit for bit.
//
// Mapping: one wavefront (one workgroup of 64) per problem.  Lane l owns the columns c = l, l + 64, ... of EVERY row: an element of `field` is only ever touched by
// its owner until the sweeps are done, so the field in global memory needs no cross-lane ordering, and every row access is coalesced.  The two rows a pass works on
// -- the row just finished and the current one -- are in LDS (2 W words), blocked cells marked, so that a lane reads its three upper neighbours and the freedom of
// its left / right neighbours (the no-corner-cutting rule) from there.  The closure of a row (min-plus along its runs of free cells) is, per 64 columns, a segmented
// min scan over the lanes on D + 5 (4096 - c) left to right and on D + 5 c right to left -- the segment a lane belongs to comes from one ballot of the blocked cells,
// no flag is scanned -- with one wave-uniform carry from chunk to chunk.  "No cell changed" is a wave-wide __any in wave-uniform control flow.
// The trace fetches the eight neighbours with eight lanes and picks the first match by ballot.  It runs twice: once for L, the arc length S and path_cells, once
// more to place the n rows of the trajectory on the polyline (there is no room to keep a path of up to H W cells, and the walk is deterministic); in the second
// walk lane l places rows l, l + 64, ... as the segment they fall in comes by.
// Every loop is bounded by max_sweeps, H, W or H W.  No atomics, nothing allocated or synchronised.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dgp_status.h"
#include "dgp_launch.h"

#pragma clang fp contract(off)

namespace {

using dgp_host::fail;

constexpr uint32_t INF = 0xffffffffu;      // unreached (and, in `field`, blocked)
constexpr uint32_t BLK = 0xfffffffeu;      // a blocked cell in the LDS rows
constexpr int MAX_SIDE = 1 << 12;
constexpr uint32_t KEY_OFF = 5u * MAX_SIDE;      // finite D < 7 * 2^24: D + KEY_OFF stays far below BLK

struct PathArgs {
  const void* sdf;
  int64_t sdf_bstride;
  int32_t H, W, B, n;
  const int32_t* env_index;      // (B) or null
  const void *start, *goal;
  void* th_init;
  uint32_t* field;
  int32_t *path_cells, *num_cells, *info;      // each may be null
  double* length;                              // may be null
  double clearance, res, orig_x, orig_y, total_time_sec;
  int32_t max_sweeps, path_cap;
};

__device__ __forceinline__ uint32_t plus(uint32_t d, uint32_t cost) { return d == INF ? INF : d + cost; }      // INF + cost = INF

// One row of a pass: the moves from `prev` (the finished row above / below; null for the first row of the pass), then the closure.  cur / prev: LDS rows of W words.
template <typename IO>
__device__ __forceinline__ bool relax_row(const PathArgs& a, const IO* __restrict__ srow, uint32_t* frow, uint32_t* cur, const uint32_t* prev, int lane) {
  const int W = a.W, NC = (W + 63) >> 6;
  for (int k = 0; k < NC; ++k) {
    const int c = k * 64 + lane;
    if (c < W) cur[c] = (double)srow[c] > a.clearance ? frow[c] : BLK;
  }
  __syncthreads();
  if (prev != nullptr) {
    for (int k = 0; k < NC; ++k) {
      const int c = k * 64 + lane;
      if (c < W) {
        uint32_t d = cur[c];
        const uint32_t up = prev[c];
        if (d != BLK && up != BLK) {      // (a blocked cell above: no axis move, and both diagonals would cut its corner)
          d = min(d, plus(up, 5u));
          if (c > 0) {
            const uint32_t pl = prev[c - 1];
            if (pl != BLK && cur[c - 1] != BLK) d = min(d, plus(pl, 7u));
          }
          if (c + 1 < W) {
            const uint32_t pr = prev[c + 1];
            if (pr != BLK && cur[c + 1] != BLK) d = min(d, plus(pr, 7u));
          }
          cur[c] = d;      // (the neighbours read this slot for `!= BLK` only, which no relaxation changes)
        }
      }
    }
    __syncthreads();      // (the next row writes its cells over `prev`)
  }
  // closure, left to right: from here on a lane touches its own slots only
  uint32_t carry = INF;
  for (int k = 0; k < NC; ++k) {
    const int c = k * 64 + lane;
    const uint32_t d = c < W ? cur[c] : BLK;
    const uint64_t blocked = __ballot(d == BLK);
    const uint64_t at_or_left = blocked & (~0ull >> (63 - lane));
    const int lb = at_or_left != 0 ? 63 - __builtin_clzll(at_or_left) : -1;      // the nearest blocked lane at or left of this one
    uint32_t key = d >= BLK ? INF : d + (KEY_OFF - 5u * (uint32_t)c);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(key, off);
      if (lane - off > lb) key = min(key, o);
    }
    if (lb < 0) key = min(key, carry);
    carry = __shfl(key, 63);
    if (d != BLK && key != INF) cur[c] = key - (KEY_OFF - 5u * (uint32_t)c);
  }
  // right to left, and the row goes back to the field
  bool changed = false;
  carry = INF;
  for (int k = NC - 1; k >= 0; --k) {
    const int c = k * 64 + lane;
    const uint32_t d = c < W ? cur[c] : BLK;
    const uint64_t blocked = __ballot(d == BLK);
    const uint64_t at_or_right = blocked >> lane;
    const int rb = at_or_right != 0 ? lane + __builtin_ctzll(at_or_right) : 64;
    uint32_t key = d >= BLK ? INF : d + 5u * (uint32_t)c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_down(key, off);
      if (lane + off < rb) key = min(key, o);
    }
    if (rb == 64) key = min(key, carry);
    carry = __shfl(key, 0);
    if (d != BLK) {
      const uint32_t out = key == INF ? INF : key - 5u * (uint32_t)c;
      cur[c] = out;
      if (out != frow[c]) { frow[c] = out; changed = true; }
    }
  }
  return changed;
}

// the eight neighbours in the order of the trace: (0,+1), (-1,0), (0,-1), (+1,0), (-1,+1), (-1,-1), (+1,-1), (+1,+1); two bits each, value + 1
__device__ __forceinline__ int nb_dr(int j) { return (int)((0xA091u >> (2 * j)) & 3u) - 1; }
__device__ __forceinline__ int nb_dc(int j) { return (int)((0x8246u >> (2 * j)) & 3u) - 1; }

// The trace: visit(index, r, c) for every traced cell, the start cell first -> L.  Wave-uniform control flow.
template <typename IO, typename F>
__device__ __forceinline__ int walk(const PathArgs& a, const IO* __restrict__ grid, const uint32_t* fld, int r, int c, int lane, F&& visit) {
  const int H = a.H, W = a.W, max_cells = H * W;
  uint32_t dcur = fld[r * W + c];
  int L = 0;
  for (;;) {
    visit(L, r, c);
    ++L;
    if (dcur == 0u || L >= max_cells) break;
    bool ok = false;
    uint32_t dn = INF;
    if (lane < 8) {
      const int dr = nb_dr(lane), dc = nb_dc(lane), nr = r + dr, nc = c + dc;
      if (nr >= 0 && nr < H && nc >= 0 && nc < W) {
        bool free = (double)grid[nr * W + nc] > a.clearance;
        if (dr != 0 && dc != 0) free = free && (double)grid[nr * W + c] > a.clearance && (double)grid[r * W + nc] > a.clearance;      // no corner cutting
        dn = fld[nr * W + nc];
        ok = free && dn != INF && dn + (dr != 0 && dc != 0 ? 7u : 5u) == dcur;
      }
    }
    const uint32_t m = (uint32_t)__ballot(ok) & 0xffu;
    if (m == 0u) break;      // (no descent: cannot happen in a converged field with D[start] < INF)
    const int j = __builtin_ctz(m);
    r += nb_dr(j); c += nb_dc(j);
    dcur = __shfl(dn, j);
  }
  return L;
}

template <typename IO>
__global__ void __launch_bounds__(64) init_paths_kernel(const PathArgs a) {
  extern __shared__ uint32_t s_rows[];      // 2 W words
  const int lane = (int)threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x;
  const int H = a.H, W = a.W, NC = (W + 63) >> 6, n = a.n, N = n - 1;
  const int64_t env = a.env_index != nullptr ? (int64_t)a.env_index[b] : b;
  const IO* __restrict__ grid = (const IO*)a.sdf + env * a.sdf_bstride;
  uint32_t* fld = a.field + b * (int64_t)H * W;
  const IO* so = (const IO*)a.start + b * 4;
  const IO* go = (const IO*)a.goal + b * 4;
  const double sx = (double)so[0], sy = (double)so[1], gx = (double)go[0], gy = (double)go[1];

  // the cells of the two points: clamp(floor(p + 0.5), 0, side - 1) of the lookup's pixel coordinates
  const double wmax = (double)(W - 1), hmax = (double)(H - 1);
  const int sc = (int)fmin(fmax(floor(a.orig_x + sx / a.res + 0.5), 0.0), wmax), sr = (int)fmin(fmax(floor(a.orig_y - sy / a.res + 0.5), 0.0), hmax);
  const int gc = (int)fmin(fmax(floor(a.orig_x + gx / a.res + 0.5), 0.0), wmax), gr = (int)fmin(fmax(floor(a.orig_y - gy / a.res + 0.5), 0.0), hmax);
  const bool start_free = (double)grid[sr * W + sc] > a.clearance, goal_free = (double)grid[gr * W + gc] > a.clearance;
  int flags = (start_free ? 0 : 1) | (goal_free ? 0 : 2);

  // D = INF, D[goal cell] = 0 if it is free (every element by its owner lane)
  for (int r = 0; r < H; ++r)
    for (int k = 0; k < NC; ++k) {
      const int c = k * 64 + lane;
      if (c < W) fld[r * W + c] = (goal_free && r == gr && c == gc) ? 0u : INF;
    }

  // sweeps: a down pass and an up pass, until one changed nothing
  bool changed = true;
  for (int sweep = 0; sweep < a.max_sweeps && changed; ++sweep) {
    bool ch = false;
    uint32_t *cur = s_rows, *prev = s_rows + W;
    for (int r = 0; r < H; ++r) {
      ch |= relax_row<IO>(a, grid + r * W, fld + r * W, cur, r > 0 ? prev : nullptr, lane);
      uint32_t* t = cur; cur = prev; prev = t;
    }
    for (int r = H - 1; r >= 0; --r) {
      ch |= relax_row<IO>(a, grid + r * W, fld + r * W, cur, r < H - 1 ? prev : nullptr, lane);
      uint32_t* t = cur; cur = prev; prev = t;
    }
    changed = __any(ch) != 0;
  }
  __threadfence();      // the trace reads the field across lanes
  __syncthreads();
  const uint32_t dstart = fld[sr * W + sc];
  if (changed) flags |= 8;
  else if (dstart == INF) flags |= 4;

  IO* th = (IO*)a.th_init + b * (int64_t)n * 4;
  int32_t* cells = a.path_cells != nullptr ? a.path_cells + b * (int64_t)a.path_cap : nullptr;
  const double vx = (gx - sx) / a.total_time_sec, vy = (gy - sy) / a.total_time_sec;
  const double Nd = (double)N;
  int L = 0;
  double S;
  if (flags != 0) {
    // the straight line of dgp_sample_problems (planner_utils.py:47-56), its formula and operation order
    const double dx = gx - sx, dy = gy - sy;
    S = sqrt(dx * dx + dy * dy);
    for (int e = lane; e < n * 4; e += 64) {
      const int i = e >> 2, cc = e & 3;
      const double s = (cc & 1) ? sy : sx, g = (cc & 1) ? gy : gx;
      const double pos = s * (double)(N - i) * 1.0 / Nd * 1.0 + g * (double)i * 1.0 / Nd * 1.0;
      const double vel = (g - s) / a.total_time_sec * 1.0;
      th[e] = (IO)(cc < 2 ? pos : vel);
    }
  } else {
    // first walk: L, the arc length, path_cells
    double px = sx, py = sy, s = 0.0;
    L = walk<IO>(a, grid, fld, sr, sc, lane, [&](int idx, int r, int c) {
      const double x = ((double)c - a.orig_x) * a.res, y = (a.orig_y - (double)r) * a.res;
      const double dx = x - px, dy = y - py;
      s = s + sqrt(dx * dx + dy * dy);
      px = x; py = y;
      if (cells != nullptr && lane == 0 && idx < a.path_cap) cells[idx] = r * W + c;
    });
    {
      const double dx = gx - px, dy = gy - py;
      s = s + sqrt(dx * dx + dy * dy);
    }
    S = s;
    if (L > a.path_cap) flags |= 16;
    // second walk: lane l places rows l, l + 64, ... < N; row i lies on segment j, the lowest j with s_{j+1} >= t_i = S i / N
    int i = lane;
    px = sx; py = sy; s = 0.0;
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
    walk<IO>(a, grid, fld, sr, sc, lane, [&](int, int r, int c) {
      const double x = ((double)c - a.orig_x) * a.res, y = (a.orig_y - (double)r) * a.res;
      s = segment(x, y);
      px = x; py = y;
    });
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
  }
  if (cells != nullptr)
    for (int k = min(L, a.path_cap) + lane; k < a.path_cap; k += 64) cells[k] = -1;
  if (lane == 0) {
    if (a.num_cells != nullptr) a.num_cells[b] = L;
    if (a.length != nullptr) a.length[b] = S;
    if (a.info != nullptr) a.info[b] = flags;
  }
}

}  // namespace

extern "C" int dgp_init_paths(const DgpHandle* h, int32_t batch, const DgpSdf* sdf, const int32_t* env_index, const DgpPathParams* p, const void* start,
                              const void* goal, void* th_init, uint32_t* field, int32_t* path_cells, int32_t* num_cells, double* length, int32_t* info,
                              void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  dgp_dev::RowMajorGrid g;
  const int rc = dgp_dev::rowmajor_grid("dgp_init_paths", h, batch, sdf, p, "DgpPathParams", start && goal && th_init && field, "start, goal, th_init and field", MAX_SIDE, g);
  if (rc != DGP_OK) return rc;
  const DgpConfig& c = *g.cfg;
  if (p->max_sweeps < 1 || p->max_sweeps > 4096) return fail(DGP_EINVAL, "dgp_init_paths: max_sweeps must be in 1..4096, got %d", p->max_sweeps);
  if (p->path_cap < 0) return fail(DGP_EINVAL, "dgp_init_paths: path_cap must be >= 0, got %d", p->path_cap);
  if (!(p->clearance == p->clearance)) return fail(DGP_EINVAL, "dgp_init_paths: NaN clearance");
  PathArgs a;
  a.sdf = sdf->data; a.sdf_bstride = sdf->batch_stride; a.H = sdf->rows; a.W = sdf->cols; a.B = batch; a.n = c.num_states;
  a.env_index = env_index; a.start = start; a.goal = goal; a.th_init = th_init; a.field = field;
  a.path_cells = path_cells; a.num_cells = num_cells; a.info = info; a.length = length;
  a.clearance = p->clearance;
  a.res = g.res; a.orig_x = g.orig_x; a.orig_y = g.orig_y;
  a.total_time_sec = c.total_time_sec;
  a.max_sweeps = p->max_sweeps; a.path_cap = p->path_cap;
  const dim3 grid((unsigned)batch), block(64);
  const unsigned lds = 2u * (unsigned)a.W * (unsigned)sizeof(uint32_t);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = c.io_dtype == DGP_F64 ? dgp_dev::launch(init_paths_kernel<double>, grid, block, lds, s, ev, a)
                                             : dgp_dev::launch(init_paths_kernel<float>, grid, block, lds, s, ev, a);
  return dgp_dev::hip_rc(e, "dgp_init_paths");
}
