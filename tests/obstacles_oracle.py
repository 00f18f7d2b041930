"""Plain-Python restatement of dgp_obstacle_maps (include/dgpmp2_hip.h), written independently of the kernel: validity is decided the REFERENCE's way, by painting
NumPy arrays with real slices -- `map[a:b, c:d] += 1` on a copy, then `any(copy > 1)` (datasets/obst_generator.py:45-64, :89-108, :66-77, :110-126) -- so the kernel's
interval arithmetic is held to NumPy's slice semantics (negative bounds, clamping, empty slices) and not to a second copy of itself.  The placement rule takes an
iterator of candidates per obstacle: the Philox candidates of the entry point, or the candidates recorded from the reference's own random_rect / random_wall
(tests/golden/g11_obstacles.npz).  tests/test_obstacles_oracle.py holds this file against the reference's maps; tests/test_hip_obstacles.py holds the kernel against this
file bit for bit."""
import math

import numpy as np

from problems_oracle import M32, philox4x32_10

RECT, WALL = 0, 1
MAX_BOXES, MAX_POINTS = 64, 32
COUNT_STREAM = 0xffffffff


class Gen(object):
  """One generator: DgpObstacleParams.  A wall reads h_min / h_max as its gap widths and start_y as gap_y."""

  def __init__(self, kind, n_lo, n_hi, w_min, w_max, h_min, h_max, start_x=0, start_y=0, end_x=0, end_y=0, patch_size=0.0, patch_size_obs=0.0, max_draws=4096):
    self.kind = {'rect': RECT, 'wall': WALL}.get(kind, kind)
    self.n_lo, self.n_hi, self.w_min, self.w_max, self.h_min, self.h_max = int(n_lo), int(n_hi), int(w_min), int(w_max), int(h_min), int(h_max)
    self.start_x, self.start_y, self.end_x, self.end_y, self.max_draws = int(start_x), int(start_y), int(end_x), int(end_y), int(max_draws)
    self.patch_size, self.patch_size_obs = float(patch_size), float(patch_size_obs)


def half(v):
  return int(math.ceil(v / 2))      # Python 3: a true division, a true ceiling


# ---- what a candidate paints: the reference's slices, with whatever signs the bounds have ----------------------------------------------------------------------------

def rect_slices(c, pad=0):
  """ObstacleRectangle._add_to_map (:72-77); c = (w, h, cx, cy) -> [(row slice, column slice)]"""
  w, h, cx, cy = c
  return [(slice(int(cy - half(h) - pad), int(cy + half(h) + pad)), slice(int(cx - half(w) - pad), int(cx + half(w) + pad)))]


def wall_slices(c):
  """ObstacleWall._add_to_map (:115-126); c = (w, gw, cx, gy) -> two (row slice, column slice)"""
  w, gw, cx, gy = c
  cols = slice(int(cx) - int(half(w)), int(cx) + int(half(w)))
  return [(slice(0, int(gy) - int(half(gw))), cols), (slice(int(gy) + int(half(gw)), None), cols)]


def point_slices(pt, pad):
  """_add_point_to_map (:66-69); pt = (x, y)"""
  return [(slice(int(math.ceil(pt[1]) - pad), int(math.ceil(pt[1]) + pad)), slice(int(math.ceil(pt[0]) - pad), int(math.ceil(pt[0]) + pad)))]


def paint(m, slices):
  for rs, cs in slices: m[rs, cs] += 1
  return m


def has_negative_bound(slices):
  return any(v is not None and v < 0 for rs, cs in slices for v in (rs.start, rs.stop, cs.start, cs.stop))


def painted_boxes(slices, H, W):
  """[r0, r1, c0, c1] of every slice pair as Python itself resolves it (slice.indices)"""
  return [list(rs.indices(H)[:2]) + list(cs.indices(W)[:2]) for rs, cs in slices]


def is_valid(m, gen, c, start_pts, goal_pts):
  """the three checks of :208-211 / :255-258, each on copies of the map"""
  pad_obs, pad_pt = half(gen.patch_size_obs), half(gen.patch_size)
  body = wall_slices(c) if gen.kind == WALL else rect_slices(c)
  grown = body if gen.kind == WALL else rect_slices(c, pad_obs)
  ok = not np.any(paint(m.copy(), grown) > 1)                        # _obstacle_collision_check
  for pts in (start_pts, goal_pts):                                   # _point_collision_check, twice
    if pts is None: continue
    with_body = paint(m.copy(), body)
    for pt in pts:
      if np.any(paint(with_body.copy(), point_slices(pt, pad_pt)) > 1):
        ok = False
        break
  return ok


def place(H, W, gen, n, candidates_of, start_pts=None, goal_pts=None):
  """The reference's placement loop (:205-212, :252-259) with the loop of every obstacle stopped after gen.max_draws candidates.  candidates_of(i): an iterator of
  the candidates of obstacle i, (w, h, cx, cy) or (w, gw, cx, gy).  -> (count map (H, W) int32, boxes [[r0, r1, c0, c1]], draws [accepted k], info)"""
  m = np.zeros((H, W), np.int32)
  boxes, draws, info = [], [], 0
  pad_pt = half(gen.patch_size)
  for pts in (start_pts, goal_pts):
    if pts is not None and any(has_negative_bound(point_slices(pt, pad_pt)) for pt in pts): info |= 4
  for i in range(n):
    it = candidates_of(i)
    k = 0
    while True:
      c = next(it)
      if is_valid(m, gen, c, start_pts, goal_pts): break
      if k == gen.max_draws - 1:
        info |= 1
        break
      k += 1
    body = wall_slices(c) if gen.kind == WALL else rect_slices(c)
    if has_negative_bound(body) or (gen.kind == RECT and has_negative_bound(rect_slices(c, half(gen.patch_size_obs)))): info |= 4
    paint(m, body)
    boxes += painted_boxes(body, H, W)
    draws.append(k)
  if np.any(m > 1): info |= 2
  return m, boxes, draws, info


# ---- the entry point's candidates -------------------------------------------------------------------------------------------------------------------------------------

def draw_in(w, a, b):
  return a + ((w * (b - a + 1)) >> 32)


def words(seed, env, k, stream):
  return philox4x32_10((env & M32, (env >> 32) & M32, k, stream), (seed & M32, (seed >> 32) & M32))


def candidate(gen, H, W, seed, env, obstacle, k):
  w = words(seed, env, k, obstacle)
  ww, hh = draw_in(w[0], gen.w_min, gen.w_max), draw_in(w[1], gen.h_min, gen.h_max)
  x_hi, y_hi = (W, H) if gen.kind == WALL else (gen.end_x, gen.end_y)
  return ww, hh, draw_in(w[2], gen.start_x + half(ww), x_hi - half(ww)), draw_in(w[3], gen.start_y + half(hh), y_hi - half(hh))


def count_and_generator(gens, seed, env):
  w = words(seed, env, 0, COUNT_STREAM)
  gen = gens[(w[1] * len(gens)) >> 32]
  return gen.n_lo + ((w[0] * (gen.n_hi - gen.n_lo)) >> 32), gen


def generate_one(gens, H, W, seed, env, start_pts=None, goal_pts=None):
  n, gen = count_and_generator(gens, seed, env)

  def candidates_of(i):
    k = 0
    while True:
      yield candidate(gen, H, W, seed, env, i, k)
      k += 1
  return place(H, W, gen, n, candidates_of, start_pts, goal_pts)


def generate(gens, E, H, W, seed=0, first_env=0, start_pts=None, goal_pts=None):
  """gens: a Gen or a sequence of them; start_pts / goal_pts (E, P, 2) or None.
  -> count (E, H, W) int32 (the images are 1 - count, or count == 0 for uint8), boxes (E, 64, 4), num_boxes (E), draws (E, 64), info (E), all int32"""
  if isinstance(gens, Gen): gens = [gens]
  count = np.zeros((E, H, W), np.int32)
  boxes, draws = np.zeros((E, MAX_BOXES, 4), np.int32), np.full((E, MAX_BOXES), -1, np.int32)
  num_boxes, info = np.zeros(E, np.int32), np.zeros(E, np.int32)
  for e in range(E):
    sp = None if start_pts is None or start_pts.shape[1] == 0 else start_pts[e]
    gp = None if goal_pts is None or goal_pts.shape[1] == 0 else goal_pts[e]
    m, bx, dr, fl = generate_one(gens, H, W, seed, first_env + e, sp, gp)
    count[e], num_boxes[e], info[e] = m, len(bx), fl
    if bx: boxes[e, :len(bx)] = bx
    draws[e, :len(dr)] = dr
  return count, boxes, num_boxes, draws, info


def image_of(count, dtype):
  """the image the entry point writes for a count map"""
  return (count == 0).astype(np.uint8) if np.dtype(dtype) == np.uint8 else (1 - count).astype(dtype)
