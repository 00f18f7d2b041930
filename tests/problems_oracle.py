"""Plain-Python fp64 restatement of dgp_sample_problems (include/dgpmp2_hip.h), written independently of the kernel: its own Philox4x32-10, its own bilinear lookup
(Env2D.get_signed_obstacle_distance, env/env_2d.py:119-175) and the reference's two rejection loops as plain sequential loops
(datasets/generate_optimal_paths_gpmp2.py:54-81, :120-162), one candidate at a time.  Python floats are IEEE binary64 and Python never contracts a * b + c, so every
comparison below is decided exactly as the reference decides it.  tests/test_problems_oracle.py holds this file against the reference's own verdicts
(tests/golden/g10_problems.npz); tests/test_hip_problems.py holds the kernel against this file bit for bit."""
import math

import numpy as np

M32 = 0xffffffff
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
  """Philox4x32 with 10 rounds (Salmon et al., SC'11; Random123): counter 4 words, key 2 words -> 4 words."""
  c0, c1, c2, c3 = [int(v) & M32 for v in counter]
  k0, k1 = [int(v) & M32 for v in key]
  for r in range(10):
    if r: k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
    c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
  return c0, c1, c2, c3


class Params(object):
  """DgpSampleParams + what the handle contributes (limits, total_time_sec); the defaults are the reference's constants."""

  def __init__(self, clearance, x_lims=(-5.0, 5.0), y_lims=(-5.0, 5.0), margin=0.5, min_dist_frac=0.6, near_tries=15, max_draws=4096, corner_inset=0.2,
               total_time_sec=10.0):
    self.clearance, self.margin, self.min_dist_frac, self.corner_inset = float(clearance), float(margin), float(min_dist_frac), float(corner_inset)
    self.near_tries, self.max_draws = int(near_tries), int(max_draws)
    self.x_lims, self.y_lims = (float(x_lims[0]), float(x_lims[1])), (float(y_lims[0]), float(y_lims[1]))
    self.total_time_sec = float(total_time_sec)
    self.lbx, self.lby = self.x_lims[0] + self.margin, self.y_lims[0] + self.margin
    self.ubx, self.uby = self.x_lims[1] - self.margin, self.y_lims[1] - self.margin
    wx, wy = self.ubx - self.lbx, self.uby - self.lby
    self.min_dist = self.min_dist_frac * math.sqrt(wx * wx + wy * wy)


def signed_distance(sdf, x, y, x_lims, y_lims):
  """env_2d.py:119-175 for one point; sdf: (H, W) array, row 0 = y_max."""
  H, W = sdf.shape
  x, y = float(x), float(y)
  res = (x_lims[1] - x_lims[0]) / (W * 1.)                      # :52
  orig_x, orig_y = (0 - x_lims[0] / res), (0 - y_lims[0] / res)   # :60-61
  max_d = x_lims[1] - x_lims[0]                                  # :56
  if not (x <= x_lims[1] and x >= x_lims[0] and y <= y_lims[1] and y >= y_lims[0]): return max_d      # :159-169 (a NaN is outside)
  px, py = orig_x + x / res, orig_y - y / res
  px1, py1 = int(math.floor(px)), int(math.floor(py))
  px2, py2 = px1 + 1, py1 + 1
  cl = lambda v, hi: min(max(v, 0), hi)
  px1, px2, py1, py2 = cl(px1, W - 1), cl(px2, W - 1), cl(py1, H - 1), cl(py2, H - 1)
  d11, d21, d12, d22 = float(sdf[py1, px1]), float(sdf[py1, px2]), float(sdf[py2, px1]), float(sdf[py2, px2])
  wa = (float(px2) - px) * (float(py2) - py)      # the clamped indices, as at :144-147
  wb = (px - float(px1)) * (float(py2) - py)
  wc = (float(px2) - px) * (py - float(py1))
  wd = (px - float(px1)) * (py - float(py1))
  return wa * d11 + wb * d21 + wc * d12 + wd * d22


def is_feasible(sdf, x, y, clearance, x_lims=(-5.0, 5.0), y_lims=(-5.0, 5.0)):
  return signed_distance(sdf, x, y, x_lims, y_lims) > clearance      # env_2d.py:86-90


def candidate(P, seed, problem, k, stream):
  w = philox4x32_10((problem & M32, (problem >> 32) & M32, k, stream), (seed & M32, (seed >> 32) & M32))
  u0 = float(((w[0] << 32) | w[1]) >> 11) * 2.0 ** -53
  u1 = float(((w[2] << 32) | w[3]) >> 11) * 2.0 ** -53
  return P.lbx + u0 * (P.ubx - P.lbx), P.lby + u1 * (P.uby - P.lby)


def sample_one(sdf, P, seed, problem, diagonal=-1):
  """-> (start (x, y), goal (x, y), draws (2), info)"""
  feas = lambda x, y: is_feasible(sdf, x, y, P.clearance, P.x_lims, P.y_lims)
  info = 0
  if 0 <= diagonal <= 3:      # :134-148
    lo_x, hi_x, lo_y, hi_y = P.x_lims[0] + P.corner_inset, P.x_lims[1] - P.corner_inset, P.y_lims[0] + P.corner_inset, P.y_lims[1] - P.corner_inset
    s, g = {0: ((lo_x, lo_y), (hi_x, hi_y)), 1: ((hi_x, hi_y), (lo_x, lo_y)), 2: ((hi_x, lo_y), (lo_x, hi_y)), 3: ((lo_x, hi_y), (hi_x, lo_y))}[diagonal]
    if feas(*s) and feas(*g): return s, g, (-1, -1), 0
    info |= 8
  k = 0
  while True:      # :63-67
    s = candidate(P, seed, problem, k, 0)
    if feas(*s): break
    if k == P.max_draws - 1:
      info |= 1
      break
    k += 1
  ks = k
  k, num_tries = 0, 0
  while True:      # :69-80
    g = candidate(P, seed, problem, k, 1)
    if feas(*g):
      dx, dy = g[0] - s[0], g[1] - s[1]
      if math.sqrt(dx * dx + dy * dy) >= P.min_dist: break
      if num_tries > P.near_tries:
        info |= 4
        break
      num_tries += 1
    if k == P.max_draws - 1:
      info |= 2
      break
    k += 1
  return s, g, (ks, k), info


def straight_line(s, g, n, total_time_sec):
  """utils/planner_utils.py:47-56 for one problem, python floats in the reference's operation order -> (n, 4)"""
  N = n - 1
  th = np.zeros((n, 4))
  for i in range(n):
    for c in range(2):
      th[i, c] = s[c] * (N - i) * 1.0 / N * 1.0 + g[c] * i * 1.0 / N * 1.0
      th[i, 2 + c] = (g[c] - s[c]) / total_time_sec * 1.0
  return th


def sample_problems(sdfs, P, B, seed=0, first_problem=0, env_index=None, diagonal=None):
  """sdfs (E, H, W) float64 (E = 1: shared) -> start (B,1,4), goal (B,1,4), draws (B,2) int32, info (B) int32 -- everything but th_init (see th_init_of)."""
  sdfs = np.asarray(sdfs, np.float64)
  start, goal = np.zeros((B, 1, 4)), np.zeros((B, 1, 4))
  draws, info = np.zeros((B, 2), np.int32), np.zeros(B, np.int32)
  for b in range(B):
    e = int(env_index[b]) if env_index is not None else (b if sdfs.shape[0] > 1 else 0)
    s, g, d, f = sample_one(sdfs[e], P, seed, first_problem + b, -1 if diagonal is None else int(diagonal[b]))
    start[b, 0, :2], goal[b, 0, :2], draws[b], info[b] = s, g, d, f
  return start, goal, draws, info


def th_init_of(start, goal, n, total_time_sec):
  return np.stack([straight_line(start[b, 0, :2], goal[b, 0, :2], n, total_time_sec) for b in range(start.shape[0])])
