// obstacle_maps.hip -- dgp_obstacle_maps: random obstacle maps (occupancy images) for a batch of environments in ONE launch (gfx950 / CDNA4).
//
// What it replaces: the reference's obstacle-map generators, one Python rejection loop per obstacle that copies and repaints the whole map for every candidate --
// generate_rect_obstacle_map / generate_wall_obstacle_map (datasets/obst_generator.py:179-221, :226-268) over random_rect / random_wall (:130-146), the three
// collision checks (:45-64, :89-108) and the slices of _add_to_map / _add_point_to_map (:66-77, :110-126), driven by get_tarpit / get_forest / get_multi_obs /
// get_passage (datasets/generate_2d_dataset.py:29-75).  include/dgpmp2_hip.h states the rule.
//
// One workgroup of four wavefronts per environment, two phases:
//   1. Placement (wavefront 0; latency-bound).  Every painted region is an axis-aligned box, so "after adding this to a copy of the map no cell exceeds 1" is a set of
//      interval-overlap tests: no map is painted to decide it.  Lane i of the wavefront keeps box i of the list (at most 64) and keep-out patch i (at most 32 + 32) in
//      registers; a round evaluates the 64 candidates k0 .. k0 + 63 of the current obstacle, one per lane, each against the placed boxes (read lane by lane, a
//      wave-uniform loop) and the patches; a ballot gives the lowest valid k -- the sequential rule, since candidate k is a pure function of (seed, environment,
//      obstacle, k) (Philox4x32-10).  The slices follow NumPy: a negative bound has the axis length added, both bounds are clamped to [0, N], start >= stop is empty --
//      a padded box that sticks out over the low edge is an EMPTY slice and its check is vacuous, as in the reference.  Once two placed boxes overlap, or a placed
//      box lies on a keep-out patch, the reference can accept nothing any more (its map copy holds a 2 whatever the candidate): every further obstacle takes its
//      last candidate, k = max_draws - 1, without evaluating the others.
//   2. Painting (all four wavefronts; memory-bound).  The list goes to LDS behind one workgroup barrier.  Rows are dealt to lane groups just wide enough for a row of
//      16-byte chunks (a 256-pixel u8 row: 16 lanes, four rows per wavefront instruction); the boxes that meet a row are selected once per row by a ballot over the
//      list (lane i tests box i), and a lane visits only those.  Chunks are aligned in memory, not to the row: a row of any width, at any offset, is written with
//      full 16-byte stores in its interior and element stores in the chunks that stick out at either end.  Every store is inside the image: boxes are clipped
//      when they are formed, elements outside [0, W) of a row are masked.
// No atomics, nothing allocated or synchronised.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "dgp_launch.h"
#include "dgp_philox.h"

namespace {

using dgp_host::fail;
using dgp::philox4x32_10;

constexpr int MAXB = DGP_OBST_MAX_BOXES, MAXP = DGP_OBST_MAX_POINTS, MAXG = DGP_OBST_MAX_GENERATORS;
constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int LIM = 1 << 20;      // bound on every size and coordinate of a generator and on the image sides: the interval arithmetic stays far inside int32
static_assert(MAXB == 64 && 2 * MAXP <= 64, "one box and one patch per lane");

struct Gen {      // DgpObstacleParams with the paddings as integers; a wall reads h_* as its gap widths and start_y as gap_y
  int32_t kind, n_lo, n_hi, w_min, w_max, h_min, h_max, start_x, start_y, end_x, end_y, max_draws, pad_obs, pad_pt;
};

struct ObstArgs {
  Gen g[MAXG];
  int32_t num_gen, H, W, P, group_shift;      // group_shift: log2 of the lanes that paint one row
  const double *start_pts, *goal_pts;        // (E, P, 2) or null
  void* image;
  int32_t *boxes, *num_boxes, *draws, *info;
  uint64_t first_env;
  uint32_t key0, key1;
};
static_assert(sizeof(ObstArgs) <= 4096, "kernel-argument segment");

struct Box { int r0, r1, c0, c1; };      // rows [r0, r1) x columns [c0, c1); empty where r0 >= r1 or c0 >= c1

// an integer of the inclusive range [a, b] from one word
__device__ __forceinline__ int draw_in(uint32_t w, int a, int b) { return a + (int)(((uint64_t)w * (uint32_t)(b - a + 1)) >> 32); }
__device__ __forceinline__ int half_up(int v) { return (v + 1) >> 1; }      // ceil(v / 2), v >= 0

// one bound of a NumPy slice on an axis of length N
__device__ __forceinline__ int bound(int v, int N, bool& wrapped) {
  if (v < 0) { v += N; wrapped = true; }
  return min(max(v, 0), N);
}
__device__ __forceinline__ Box slice(int r0, int r1, int c0, int c1, int H, int W, bool& wrapped) {
  Box b;
  b.r0 = bound(r0, H, wrapped); b.r1 = bound(r1, H, wrapped); b.c0 = bound(c0, W, wrapped); b.c1 = bound(c1, W, wrapped);
  return b;
}
__device__ __forceinline__ bool meets(const Box& a, const Box& b) { return max(a.r0, b.r0) < min(a.r1, b.r1) && max(a.c0, b.c0) < min(a.c1, b.c1); }
__device__ __forceinline__ Box box_of_lane(const Box& v, int src) {      // src: wave-uniform
  Box b;
  b.r0 = __builtin_amdgcn_readlane(v.r0, src); b.r1 = __builtin_amdgcn_readlane(v.r1, src);
  b.c0 = __builtin_amdgcn_readlane(v.c0, src); b.c1 = __builtin_amdgcn_readlane(v.c1, src);
  return b;
}
__device__ __forceinline__ int ceil_to_int(double v) { return (int)fmin(fmax(ceil(v), -1073741824.0), 1073741824.0); }

struct Candidate { Box u0, u1, p0, p1; bool wrapped; };      // the boxes as painted (a rectangle: u1 empty), the boxes of the obstacle check (a rectangle: padded)

// candidate k of obstacle `obstacle` of environment `env`
__device__ __forceinline__ Candidate candidate(const ObstArgs& a, const Gen& g, uint64_t env, uint32_t obstacle, uint32_t k) {
  uint32_t w[4];
  philox4x32_10((uint32_t)env, (uint32_t)(env >> 32), k, obstacle, a.key0, a.key1, w);
  const int H = a.H, W = a.W;
  Candidate c;
  c.wrapped = false;
  const Box none = {0, 0, 0, 0};
  if (g.kind == DGP_OBST_WALL) {      // random_wall (:141-146), ObstacleWall._add_to_map (:115-126)
    const int ww = draw_in(w[0], g.w_min, g.w_max), gw = draw_in(w[1], g.h_min, g.h_max);
    const int w2 = half_up(ww), g2 = half_up(gw);
    const int cx = draw_in(w[2], g.start_x + w2, W - w2), gy = draw_in(w[3], g.start_y + g2, H - g2);
    c.u0 = slice(0, gy - g2, cx - w2, cx + w2, H, W, c.wrapped);
    c.u1 = slice(gy + g2, H, cx - w2, cx + w2, H, W, c.wrapped);      // `gy + g2 :` -- an omitted stop is the axis length
    c.p0 = c.u0; c.p1 = c.u1;
  } else {      // random_rect (:130-139), ObstacleRectangle._add_to_map (:72-77)
    const int ww = draw_in(w[0], g.w_min, g.w_max), hh = draw_in(w[1], g.h_min, g.h_max);
    const int w2 = half_up(ww), h2 = half_up(hh);
    const int cx = draw_in(w[2], g.start_x + w2, g.end_x - w2), cy = draw_in(w[3], g.start_y + h2, g.end_y - h2);
    c.u0 = slice(cy - h2, cy + h2, cx - w2, cx + w2, H, W, c.wrapped);
    c.p0 = slice(cy - h2 - g.pad_obs, cy + h2 + g.pad_obs, cx - w2 - g.pad_obs, cx + w2 + g.pad_obs, H, W, c.wrapped);
    c.u1 = none; c.p1 = none;
  }
  return c;
}

// ---- phase 2 -------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void paint(const ObstArgs& a, T* __restrict__ img, const Box* s_box, int nb, int tid) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int H = a.H, W = a.W;
  const int wave = tid >> 6, lane = tid & 63;
  const int gs = a.group_shift, G = 1 << gs, RPI = 64 >> gs;      // lanes per row, rows per wavefront and pass
  const int sub = lane >> gs, j0 = lane & (G - 1);
  const Box mine = s_box[lane];
  const bool live = lane < nb && mine.c0 < mine.c1;
  for (int row0 = wave * RPI; row0 < H; row0 += WAVES * RPI) {      // (wave-uniform)
    uint64_t rowmask = 0;      // the boxes that meet this lane's row
    for (int i = 0; i < RPI; ++i) {
      const int r = row0 + i;
      const uint64_t m = __ballot(live && r >= mine.r0 && r < mine.r1);
      if (i == sub) rowmask = m;
    }
    const int r = row0 + sub;
    T* rowp = img + (int64_t)r * W;
    const int mis = (int)((reinterpret_cast<uintptr_t>(rowp) & 15u) / sizeof(T));      // elements between the 16-byte boundary in front of the row and the row
    const int chunks = r < H ? (W + mis + VEC - 1) / VEC : 0;      // (a lane group past the last row stores nothing)
    for (int j = j0; j < chunks; j += G) {
      const int s = j * VEC - mis;      // the chunk holds columns s .. s + VEC - 1
      const bool full = s >= 0 && s + VEC <= W;
      if constexpr (sizeof(T) == 1) {
        uint32_t cov = 0;      // bit v: column s + v is covered
        for (uint64_t m = rowmask; m != 0; m &= m - 1) {
          const Box b = s_box[__builtin_ctzll(m)];
          const int lo = max(b.c0 - s, 0), hi = min(b.c1 - s, VEC);
          if (hi > lo) cov |= ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        }
        if (full) {
          uint32_t q[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const uint32_t n = (cov >> (4 * i)) & 15u;
            q[i] = ((n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21)) ^ 0x01010101u;      // 1 where free
          }
          *reinterpret_cast<uint4*>(rowp + s) = make_uint4(q[0], q[1], q[2], q[3]);
        } else {
          for (int v = 0; v < VEC; ++v)
            if (s + v >= 0 && s + v < W) rowp[s + v] = (T)(((cov >> v) & 1u) ^ 1u);
        }
      } else {
        int cnt[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) cnt[v] = 0;
        for (uint64_t m = rowmask; m != 0; m &= m - 1) {
          const Box b = s_box[__builtin_ctzll(m)];
#pragma unroll
          for (int v = 0; v < VEC; ++v) cnt[v] += (s + v >= b.c0 && s + v < b.c1) ? 1 : 0;
        }
        if (full) {
          T val[VEC];
#pragma unroll
          for (int v = 0; v < VEC; ++v) val[v] = (T)(1 - cnt[v]);      // the reference's 1 - obst_map
          uint4 q;
          __builtin_memcpy(&q, val, 16);
          *reinterpret_cast<uint4*>(rowp + s) = q;
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            if (s + v >= 0 && s + v < W) rowp[s + v] = (T)(1 - cnt[v]);
        }
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(TPB) obstacle_maps_kernel(const ObstArgs a) {
  __shared__ Box s_box[MAXB];
  __shared__ int s_nb;
  const int tid = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x;
  const int H = a.H, W = a.W;

  if (tid < 64) {      // ---- phase 1: wavefront 0 places the obstacles ----
    const int lane = tid;
    const uint64_t env = a.first_env + (uint64_t)e;
    uint32_t w[4];
    philox4x32_10((uint32_t)env, (uint32_t)(env >> 32), 0u, 0xffffffffu, a.key0, a.key1, w);
    const int gi = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[1] * (uint32_t)a.num_gen) >> 32));      // np.random.choice(range(num_gen))
    const Gen& g = a.g[gi];
    const int n = __builtin_amdgcn_readfirstlane(g.n_lo + (int)(((uint64_t)w[0] * (uint32_t)(g.n_hi - g.n_lo)) >> 32));      // np.random.randint(n_lo, n_hi)
    const int per = g.kind == DGP_OBST_WALL ? 2 : 1;
    const uint32_t max_draws = (uint32_t)g.max_draws;

    // keep-out patches (_add_point_to_map, :66-69): lane i < ns the start points, then the goal points
    const int ns = a.start_pts != nullptr ? a.P : 0, np = ns + (a.goal_pts != nullptr ? a.P : 0);
    Box patch = {0, 0, 0, 0};
    bool pwrap = false;
    if (lane < np) {
      const double* pt = lane < ns ? a.start_pts + (e * a.P + lane) * 2 : a.goal_pts + (e * a.P + (lane - ns)) * 2;
      const int px = ceil_to_int(pt[0]), py = ceil_to_int(pt[1]);
      patch = slice(py - g.pad_pt, py + g.pad_pt, px - g.pad_pt, px + g.pad_pt, H, W, pwrap);
    }
    int flags = __any(pwrap) ? 4 : 0;

    Box mine = {0, 0, 0, 0};      // box `lane` of the list
    int my_draw = -1;             // accepted k of obstacle `lane`
    int nb = 0;
    bool over = false;            // two placed boxes overlap: the finished map holds a cell > 1
    bool blocked = false;         // ... or a placed box lies on a patch: whatever the candidate, the reference's map copy holds a cell > 1
    for (int i = 0; i < n; ++i) {
      uint32_t acc_k = max_draws - 1u;
      Candidate acc;
      bool capped = true;
      if (blocked) acc = candidate(a, g, env, (uint32_t)i, acc_k);
      else
        for (uint32_t k0 = 0;; k0 += 64u) {
          const uint32_t k = k0 + (uint32_t)lane;
          const Candidate c = candidate(a, g, env, (uint32_t)i, k);
          bool ok = k < max_draws && !meets(c.u0, c.u1);      // (a wall whose first slice wrapped may lie on its second)
          for (int j = 0; j < nb; ++j) {
            const Box b = box_of_lane(mine, j);
            ok = ok && !meets(c.p0, b) && !meets(c.p1, b);                       // _obstacle_collision_check (:45-50, :89-94)
            if (np > 0) ok = ok && !meets(c.u0, b) && !meets(c.u1, b);           // _point_collision_check paints the box without padding (:55, :99)
          }
          for (int j = 0; j < np; ++j) {
            const Box q = box_of_lane(patch, j);
            ok = ok && !meets(c.u0, q) && !meets(c.u1, q);                       // :56-60, :100-104
          }
          const uint64_t vm = __ballot(ok);
          const bool last = max_draws - k0 <= 64u;
          if (vm != 0 || last) {
            const int src = vm != 0 ? (int)__builtin_ctzll(vm) : (int)(max_draws - 1u - k0);      // nothing valid in the last round: the last candidate drawn
            acc.u0 = box_of_lane(c.u0, src); acc.u1 = box_of_lane(c.u1, src);
            acc.wrapped = __builtin_amdgcn_readlane((int)c.wrapped, src) != 0;
            acc_k = k0 + (uint32_t)src;
            capped = vm == 0;
            break;
          }
        }
      // obst_map = _add_to_map(obst_map) (:212, :259)
      const bool hit = lane < nb && (meets(mine, acc.u0) || meets(mine, acc.u1));
      over = over || __any(hit) || meets(acc.u0, acc.u1);
      blocked = blocked || over || __any(lane < np && (meets(patch, acc.u0) || meets(patch, acc.u1)));
      if (lane == nb) mine = acc.u0;
      if (per == 2 && lane == nb + 1) mine = acc.u1;
      if (lane == i) my_draw = (int)acc_k;
      nb += per;
      flags |= (capped ? 1 : 0) | (acc.wrapped ? 4 : 0);
    }
    if (over) flags |= 2;
    if (lane >= nb) mine = Box{0, 0, 0, 0};
    s_box[lane] = mine;
    if (lane == 0) s_nb = nb;
    if (a.boxes != nullptr) {
      int32_t* o = a.boxes + (e * MAXB + lane) * 4;
      o[0] = mine.r0; o[1] = mine.r1; o[2] = mine.c0; o[3] = mine.c1;
    }
    if (a.draws != nullptr) a.draws[e * MAXB + lane] = lane < n ? my_draw : -1;
    if (lane == 0) {
      if (a.num_boxes != nullptr) a.num_boxes[e] = nb;
      if (a.info != nullptr) a.info[e] = flags;
    }
  }
  __syncthreads();
  paint<T>(a, (T*)a.image + e * (int64_t)H * W, s_box, s_nb, tid);
}

}  // namespace

extern "C" int dgp_obstacle_maps(const DgpHandle* h, int32_t batch, int32_t rows, int32_t cols, const DgpObstacleParams* params, int32_t num_params, uint64_t seed,
                                 uint64_t first_env, const double* start_pts, const double* goal_pts, int32_t num_pts, void* image, int32_t image_dtype,
                                 int32_t* boxes, int32_t* num_boxes, int32_t* draws, int32_t* info, void* stream) {
  const dgp_dev::Events ev = dgp_dev::take_events();
  if (!h) return fail(DGP_EINVAL, "null handle");
  if (!params) return fail(DGP_EINVAL, "dgp_obstacle_maps: null DgpObstacleParams");
  if (!image) return fail(DGP_EINVAL, "dgp_obstacle_maps: image must be a non-null device pointer");
  if (batch <= 0) return fail(DGP_EINVAL, "dgp_obstacle_maps: batch must be positive, got %d", batch);
  if (rows < 1 || cols < 1 || rows > LIM || cols > LIM || (int64_t)rows * cols >= ((int64_t)1 << 31))
    return fail(DGP_EINVAL, "dgp_obstacle_maps: bad map size %d x %d", rows, cols);
  if (num_params < 1 || num_params > MAXG) return fail(DGP_EINVAL, "dgp_obstacle_maps: num_params must be in 1..%d, got %d", MAXG, num_params);
  if (image_dtype != DGP_U8 && image_dtype != DGP_F32 && image_dtype != DGP_F64) return fail(DGP_EINVAL, "dgp_obstacle_maps: bad image_dtype %d", image_dtype);
  const int esz = image_dtype == DGP_U8 ? 1 : (image_dtype == DGP_F32 ? 4 : 8);
  if (reinterpret_cast<uintptr_t>(image) % (uintptr_t)esz) return fail(DGP_EINVAL, "dgp_obstacle_maps: image is not aligned to its element size");
  const bool points = start_pts || goal_pts;
  if (num_pts < 0 || num_pts > MAXP) return fail(DGP_EINVAL, "dgp_obstacle_maps: at most %d keep-out points per list, got %d", MAXP, num_pts);
  if (points && num_pts == 0) start_pts = goal_pts = nullptr;      // (an empty list keeps nothing out)
  ObstArgs a;
  for (int i = 0; i < num_params; ++i) {
    const DgpObstacleParams& q = params[i];
    Gen& g = a.g[i];
    if (q.kind != DGP_OBST_RECT && q.kind != DGP_OBST_WALL) return fail(DGP_EINVAL, "dgp_obstacle_maps: bad generator kind %d", q.kind);
    const bool wall = q.kind == DGP_OBST_WALL;
    if (q.n_lo < 0 || q.n_hi <= q.n_lo) return fail(DGP_EINVAL, "dgp_obstacle_maps: the obstacle count range [%d, %d) is empty", q.n_lo, q.n_hi);
    if ((int64_t)(q.n_hi - 1) * (wall ? 2 : 1) > MAXB)
      return fail(DGP_EINVAL, "dgp_obstacle_maps: up to %d obstacles of %d box(es): more than %d boxes", q.n_hi - 1, wall ? 2 : 1, MAXB);
    if (q.max_draws < 1) return fail(DGP_EINVAL, "dgp_obstacle_maps: max_draws must be >= 1, got %d", q.max_draws);
    if (q.w_min < 0 || q.w_max < q.w_min || q.w_max > LIM || q.h_min < 0 || q.h_max < q.h_min || q.h_max > LIM)
      return fail(DGP_EINVAL, "dgp_obstacle_maps: bad size ranges [%d, %d], [%d, %d]", q.w_min, q.w_max, q.h_min, q.h_max);
    if (abs(q.start_x) > LIM || abs(q.start_y) > LIM || abs(q.end_x) > LIM || abs(q.end_y) > LIM) return fail(DGP_EINVAL, "dgp_obstacle_maps: coordinate range out of bounds");
    if (!(q.patch_size_obs == q.patch_size_obs) || !(q.patch_size == q.patch_size)) return fail(DGP_EINVAL, "dgp_obstacle_maps: NaN padding in DgpObstacleParams");
    const double po = ceil(q.patch_size_obs / 2.0), pp = ceil(q.patch_size / 2.0);      // ceil(patch_size / 2) (:67-68, :75-76)
    if (fabs(po) > LIM || fabs(pp) > LIM) return fail(DGP_EINVAL, "dgp_obstacle_maps: padding out of bounds");
    // randint(a, b) raises where b < a: the widest obstacle must leave a centre
    const int w2 = (q.w_max + 1) / 2, h2 = (q.h_max + 1) / 2;
    const int ex = wall ? cols : q.end_x, ey = wall ? rows : q.end_y;
    if (q.start_x + w2 > ex - w2 || q.start_y + h2 > ey - h2)
      return fail(DGP_EINVAL, "dgp_obstacle_maps: empty coordinate range for the largest obstacle: x [%d, %d], y [%d, %d]", q.start_x + w2, ex - w2, q.start_y + h2, ey - h2);
    g.kind = q.kind; g.n_lo = q.n_lo; g.n_hi = q.n_hi; g.w_min = q.w_min; g.w_max = q.w_max; g.h_min = q.h_min; g.h_max = q.h_max;
    g.start_x = q.start_x; g.start_y = q.start_y; g.end_x = q.end_x; g.end_y = q.end_y; g.max_draws = q.max_draws;
    g.pad_obs = (int)po; g.pad_pt = (int)pp;
  }
  for (int i = num_params; i < MAXG; ++i) a.g[i] = a.g[0];
  a.num_gen = num_params; a.H = rows; a.W = cols; a.P = num_pts;
  const int vec = 16 / esz;
  const bool rows_aligned = reinterpret_cast<uintptr_t>(image) % 16 == 0 && cols % vec == 0;      // every row of every map starts on a 16-byte boundary
  const int max_chunks = rows_aligned ? cols / vec : (cols + 2 * vec - 2) / vec;      // chunks of a row, at the worst misalignment
  a.group_shift = 0;
  while ((1 << a.group_shift) < max_chunks && a.group_shift < 6) ++a.group_shift;
  a.start_pts = start_pts; a.goal_pts = goal_pts;
  a.image = image; a.boxes = boxes; a.num_boxes = num_boxes; a.draws = draws; a.info = info;
  a.first_env = first_env;
  a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32);
  const dim3 grid((unsigned)batch), block(TPB);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t er = image_dtype == DGP_U8 ? dgp_dev::launch(obstacle_maps_kernel<uint8_t>, grid, block, 0, s, ev, a)
                        : (image_dtype == DGP_F32 ? dgp_dev::launch(obstacle_maps_kernel<float>, grid, block, 0, s, ev, a)
                                                  : dgp_dev::launch(obstacle_maps_kernel<double>, grid, block, 0, s, ev, a));
  return dgp_dev::hip_rc(er, "dgp_obstacle_maps");
}
