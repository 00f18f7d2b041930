"""Inputs of the initial-path tests (tests/test_paths_oracle.py, tests/test_hip_paths.py): hand-built maps at the smallest sizes where dgp_init_paths can go wrong, and
the oracle's answer for them (tests/paths_oracle.py), computed once per group and shared read-only.

A GROUP is a stack of maps of one size with the problems posed in them (one launch with env_index).  Signed distance fields come from oracle.edt_oracle.sdf_2d
(image 1 = free; scipy's identical transform for the larger maps), so they are what sdf_2d_batch makes of such a map; the structural groups take clearance = half a cell: exactly the free pixels are free cells.
  g16   16 x 16            empty map (axis-aligned, diagonal, start and goal in one cell), a goal enclosed by a ring (bit 2), a start / goal on a blocked cell (bits 0, 1),
                           two blocked cells that touch diagonally between start and goal (the path must not pass between them)
  g24   24 x 40            W no multiple of 64, H != W: a wall with one gap, both ways, and a goal on the last row AND column
  g64   64 x 64            a U-shaped trap (the path first runs away from the goal), a serpentine of 5 teeth (several sweeps; with max_sweeps = 1: bit 3)
  g100  100 x 130          more than one column group per lane, ragged: the serpentine across the chunk boundaries at columns 64 and 128
  g256  256 x 256          random boxes in a frame; start / goal pairs from problems_oracle.sample_problems at clearance + 0.1 (the feasibility property)
  p64   64 x 64 over [-2, 2]^2 (cells of 0.0625): boxes in a frame, pairs sampled the same way (the feasibility property)
Start and goal points sit off the cell points (a non-zero first and last segment) unless a case says otherwise."""
import collections
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)
from oracle import edt_oracle as E      # noqa: E402
import paths_oracle as PA               # noqa: E402
import problems_oracle as PO            # noqa: E402

Group = collections.namedtuple('Group', 'name H W x_lims y_lims n t_sec clearance images sdfs names env start goal')
LIMS = (-5.0, 5.0)


def _sdf_2d(im, res):
  """utils/sdf_utils.py:6-21 without padding: scipy's transform (the reference's own dependency; the brute-force oracle takes 20 s for a 256 x 256 map), which
  tests/test_sdf_edt.py holds bit-identical to oracle.edt_oracle.sdf_2d -- the small maps use that one"""
  if im.size <= 4096: return E.sdf_2d(im, padlen=0, res=res)
  from scipy import ndimage
  free = im > 0.75
  return (ndimage.distance_transform_edt(free) - ndimage.distance_transform_edt(1 - free)) * res


def _sdfs(images, x_lims):
  res = (x_lims[1] - x_lims[0]) / images.shape[2]
  return np.stack([_sdf_2d(im, res) for im in images])


def _at(r, c, W, x_lims, y_lims, off=(0.013, -0.021)):
  """a point in cell (r, c), `off` cells away from its cell point"""
  res, ox, oy = PA.geometry(W, x_lims, y_lims)
  return ((c + off[0]) - ox) * res, (oy - (r + off[1])) * res


def _group(name, images, n, problems, x_lims=LIMS, y_lims=LIMS, t_sec=10.0, clearance=None):
  """problems: (case name, map index, (x, y) start, (x, y) goal)"""
  images = np.asarray(images, np.float64)
  _, H, W = images.shape
  sdfs = _sdfs(images, x_lims)
  B = len(problems)
  start, goal = np.zeros((B, 1, 4)), np.zeros((B, 1, 4))
  for b, (_, _, s, g) in enumerate(problems): start[b, 0, :2], goal[b, 0, :2] = s, g
  if clearance is None: clearance = 0.5 * (x_lims[1] - x_lims[0]) / W
  g = Group(name, H, W, x_lims, y_lims, n, t_sec, float(clearance), images, sdfs, tuple(p[0] for p in problems), np.array([p[1] for p in problems], np.int32), start, goal)
  for a in (g.images, g.sdfs, g.env, g.start, g.goal): a.setflags(write=False)
  return g


def _serpentine(H, W, cols, gap):
  im = np.ones((H, W))
  for i, c in enumerate(cols):
    if i % 2 == 0: im[:H - gap, c] = 0.0      # a tooth from the top
    else: im[gap:, c] = 0.0                   # ... from the bottom
  return im


@functools.lru_cache(maxsize=None)
def group(name):
  at = lambda r, c, off=(0.013, -0.021): _at(r, c, W, LIMS, LIMS, off)
  if name == 'g16':
    H = W = 16
    empty, ring, diag, block = (np.ones((H, W)) for _ in range(4))
    ring[5:10, 5:10] = 0.0; ring[6:9, 6:9] = 1.0
    diag[7, 7] = diag[8, 8] = 0.0
    block[12:14, 12:14] = 0.0
    return _group(name, [empty, ring, diag, block], 7, [
        ('empty_axis', 0, at(8, 2), at(8, 13)), ('empty_diagonal', 0, at(13, 2), at(2, 13)), ('same_cell', 0, at(4, 4, (0.2, 0.1)), at(4, 4, (-0.3, -0.2))),
        ('same_point_on_cell', 0, at(9, 3, (0.0, 0.0)), at(9, 3, (0.0, 0.0))), ('enclosed_goal', 1, at(2, 2), at(7, 7)), ('start_blocked', 3, at(12, 13), at(3, 3)),
        ('goal_blocked', 3, at(3, 3), at(13, 12)), ('diagonal_touch', 2, at(8, 7), at(7, 8)), ('diagonal_touch_far', 2, at(11, 4), at(4, 11))])
  if name == 'g24':
    H, W = 24, 40
    wall, open_ = np.ones((H, W)), np.ones((H, W))
    wall[:, 20] = 0.0; wall[5:7, 20] = 1.0
    return _group(name, [wall, open_], 16, [
        ('wall_gap', 0, at(18, 4), at(17, 35)), ('wall_gap_back', 0, at(17, 35), at(18, 4)), ('goal_last_row_and_column', 0, at(2, 3), at(23, 39, (0.0, 0.0))),
        ('start_last_row_and_column', 1, at(23, 39, (-0.2, -0.2)), at(0, 0, (0.1, 0.1)))])
  if name == 'g64':
    H = W = 64
    trap = np.ones((H, W))
    trap[20:45, 40] = 0.0; trap[20, 24:41] = 0.0; trap[44, 24:41] = 0.0
    serp = _serpentine(H, W, (10, 20, 30, 40, 50), 10)
    return _group(name, [trap, serp], 64, [('u_trap', 0, at(32, 34), at(32, 52)), ('serpentine', 1, at(32, 3), at(30, 58)), ('serpentine_back', 1, at(30, 58), at(32, 3))])
  if name == 'g100':
    H, W = 100, 130
    serp = _serpentine(H, W, (20, 40, 62, 66, 100, 128), 15)      # (a corridor across the chunk boundary at column 64, a tooth on column 128)
    return _group(name, [serp], 101, [('serpentine_ragged', 0, at(50, 5), at(48, 129)), ('serpentine_ragged_back', 0, at(48, 129), at(50, 5))])
  if name in ('g256', 'p64'):
    H = W = 256 if name == 'g256' else 64
    x_lims = y_lims = LIMS if name == 'g256' else (-2.0, 2.0)
    rs = np.random.RandomState(3 if name == 'g256' else 4)
    im = np.ones((H, W))
    for _ in range(14 if name == 'g256' else 5):
      h, w = rs.randint(H // 16, H // 5, 2)
      r, c = rs.randint(0, H - h), rs.randint(0, W - w)
      im[r:r + h, c:c + w] = 0.0
    im[0] = im[-1] = 0.0; im[:, 0] = im[:, -1] = 0.0      # the frame: the reference's lookup collapses on the last row / column (clamped taps), no path may run there
    clearance = 0.2
    B = 2 if name == 'g256' else 8
    P = PO.Params(clearance + 0.1, x_lims=x_lims, y_lims=y_lims)      # the sampler's default: 0.1 above the planner's clearance
    s, g, _, sinfo = PO.sample_problems(_sdfs(im[None], x_lims), P, B, seed=21)
    assert not sinfo.any() or not (sinfo & 3).any()
    return _group(name, [im], 130 if name == 'g256' else 33, [('sampled_%d' % b, 0, tuple(s[b, 0, :2]), tuple(g[b, 0, :2])) for b in range(B)], x_lims, y_lims, 10.0, clearance)
  raise KeyError(name)


GROUPS = ('g16', 'g24', 'g64', 'g100', 'g256', 'p64')
PROPERTY_GROUPS = ('g256', 'p64')


def _round(a, io):
  return a.astype(np.float32).astype(np.float64) if io == 'f32' else a


@functools.lru_cache(maxsize=None)
def expected(name, io='f64', max_sweeps=None, path_cap=None):
  """The oracle's answer for a group as the kernel sees it with `io` tensors (fp32: grids and points rounded once on the way in) -> (dict, max_sweeps, path_cap).
  max_sweeps None: what sweep_field needed on the CPU plus a margin of 2 (the oracle alone is inside the cap); path_cap None: the longest path plus 3."""
  g = group(name)
  kw = dict(env_index=g.env, x_lims=g.x_lims, y_lims=g.y_lims, total_time_sec=g.t_sec)
  sdfs, start, goal = _round(g.sdfs, io), _round(g.start, io), _round(g.goal, io)
  if max_sweeps is None or path_cap is None:
    free_run, _, _ = expected(name, io, 64, 1 << 16)      # (a converged field does not depend on the cap, nor a path on path_cap)
    assert not (free_run['info'] & PA.BIT_UNCONVERGED).any(), name
    if max_sweeps is None: max_sweeps = int(free_run['sweeps'].max()) + 2
    if path_cap is None: path_cap = int(free_run['num_cells'].max()) + 3
    out = dict(free_run, path_cells=np.ascontiguousarray(free_run['path_cells'][:, :path_cap]))
    out['info'] = free_run['info'] | np.where(free_run['num_cells'] > path_cap, PA.BIT_TRUNCATED, 0).astype(np.int32)
  else:
    out = PA.init_paths(sdfs, start, goal, g.n, g.clearance, max_sweeps, path_cap, **kw)
  for a in out.values(): a.setflags(write=False)
  return out, max_sweeps, path_cap
