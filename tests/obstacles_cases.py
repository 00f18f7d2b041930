"""Inputs of the dgp_obstacle_maps tests, shared by tests/test_obstacles_oracle.py (CPU: the inputs take every branch and cap nowhere) and tests/test_hip_obstacles.py
(GPU: the kernel against tests/obstacles_oracle.py, bit for bit).  The oracle's result of a case is computed once per process.

Two shapes: E = 9 maps of 32 x 37 (a width that is no multiple of 4, 16 or of any vector: every row starts at another offset from a 16-byte boundary) and E = 130 maps
of 64 x 64.  The generators are the reference's four dataset types evaluated for the side (tests/golden/make_obstacles_golden.py has the same numbers), 'mixed' (one of
the first three per environment), 'forest44' (exactly 44 obstacles) and 'wrap': centres from the low edge on and a large separation, so that padded boxes stick out
over the edge, wrap and come out empty.  The forests are separated by patch_size_obs = 0 here: with a padding, a forest of a batch this size always holds a map
whose vacuous check let two obstacles overlap, after which nothing is valid and the loop runs to its cap -- `wrap` covers that path in a batch small enough for a seed
to exist that caps nowhere.  The seeds were chosen on the CPU so that the oracle flags no environment capped (test_gpu_test_inputs_cap_nowhere; test_gpu_test_inputs_take_every_branch holds the branches)."""
import functools

import numpy as np

import obstacles_oracle as OO

SMALL, MAIN = (9, 32, 37), (130, 64, 64)      # E, H, W


def gens_of(name, side):
  """the generators of a case for maps of this side (32 or 64)"""
  G = OO.Gen
  if side == 32:
    sets = {'tar_pit': G('rect', 5, 8, 3, 4, 3, 4, 4, 4, 20, 20, 4.0, 0.0), 'forest': G('rect', 23, 45, 1, 2, 1, 2, 0, 0, 31, 31, 3.0, 0.0),
            'multi_obs': G('rect', 2, 5, 4, 14, 4, 14, 3, 3, 28, 28, 2.0, 4.0), 'passage': G('wall', 1, 2, 6, 16, 4, 5, 4, 0, 0, 0, 3.0, 0.0),
            'forest44': G('rect', 44, 45, 1, 2, 1, 2, 0, 0, 31, 31, 3.0, 0.0), 'wrap': G('rect', 4, 7, 2, 5, 2, 5, 0, 0, 31, 31, 5.0, 7.0, max_draws=256)}
  else:
    sets = {'tar_pit': G('rect', 5, 8, 6, 7, 6, 7, 9, 9, 41, 41, 5.0, 0.0), 'forest': G('rect', 23, 45, 2, 3, 2, 3, 0, 0, 63, 63, 3.0, 0.0),
            'multi_obs': G('rect', 2, 5, 8, 18, 8, 18, 6, 6, 57, 57, 3.0, 6.0), 'passage': G('wall', 1, 2, 12, 22, 4, 5, 9, 0, 0, 0, 3.0, 0.0),
            'forest44': G('rect', 44, 45, 2, 3, 2, 3, 0, 0, 63, 63, 3.0, 0.0), 'wrap': G('rect', 4, 7, 4, 9, 3, 8, 0, 0, 40, 63, 4.0, 12.0, max_draws=256)}
  if name == 'mixed': return [sets['tar_pit'], sets['forest'], sets['multi_obs']]
  return [sets[name]]


# name -> (generator, shape, seed, first_env, keep-out points per list)
CASES = {
    'small_tar_pit': ('tar_pit', SMALL, 26, 0, 3),
    'small_forest': ('forest', SMALL, 2, 0, 3),
    'small_multi_obs': ('multi_obs', SMALL, 3, 0, 3),
    'small_passage': ('passage', SMALL, 4, 0, 3),
    'small_mixed': ('mixed', SMALL, 5, 0, 0),
    'small_wrap': ('wrap', SMALL, 6, 0, 2),
    'small_wrap_no_points': ('wrap', SMALL, 55, 0, 0),
    'small_forest44_high_env': ('forest44', SMALL, 7, (1 << 40) + 3, 0),
    'main_tar_pit': ('tar_pit', MAIN, 11, 0, 0),
    'main_forest': ('forest', MAIN, 12, 0, 2),
    'main_multi_obs': ('multi_obs', MAIN, 13, 0, 0),
    'main_passage': ('passage', MAIN, 14, 0, 2),
    'main_mixed': ('mixed', MAIN, 15, 1000, 2),
}


def points(name):
  """(start_pts, goal_pts), each (E, P, 2) float64 pixel coordinates (x, y) or None; the last start point of every environment sits by the low edges (its patch meets a
  negative slice bound)"""
  gen, (E, H, W), seed, first_env, P = CASES[name]
  if P == 0: return None, None
  rs = np.random.RandomState(7000 + seed)
  lo = np.array([2.0, 2.0]); hi = np.array([W - 3.0, H - 3.0])
  start, goal = rs.uniform(lo, hi, (E, P, 2)), rs.uniform(lo, hi, (E, P, 2))
  start[:, P - 1] = rs.uniform(0.05, 1.6, (E, 2))
  return start, goal


@functools.lru_cache(maxsize=None)
def expected(name):
  """the oracle's (count (E,H,W), boxes (E,64,4), num_boxes (E), draws (E,64), info (E)) of a case -- computed once, never modified (the arrays are read-only)"""
  gen, (E, H, W), seed, first_env, P = CASES[name]
  start, goal = points(name)
  out = OO.generate(gens_of(gen, 32 if H == 32 else 64), E, H, W, seed, first_env, start, goal)
  for a in out: a.setflags(write=False)
  return out
