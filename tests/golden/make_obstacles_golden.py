#!/usr/bin/env python
"""Generate tests/golden/g11_obstacles.npz: what the obstacle-map generator (dgp_obstacle_maps) must agree with, computed by the REAL reference --
generate_rect_obstacle_map / generate_wall_obstacle_map of datasets/obst_generator.py, run under random.seed with random_rect / random_wall wrapped so that every
candidate they return is recorded (w, h, cx, cy / w, gw, cx, gy, in the order drawn) next to the map that comes back.  Nothing of the reference is edited.
Only arrays are stored.  Re-run with:   python tests/golden/make_obstacles_golden.py   (the file regenerates byte for byte: fixed seeds, fixed zip timestamps)

make_golden.py / make_metrics_golden.py (imported for where the reference lives and for write_npz) are left as they are.

Cases: the parameter sets of the four dataset types (generate_2d_dataset.py:29-75 evaluated for im_size 32 and 64), each without keep-out points and with two start
and two goal points (some close enough to the low edges for their patches to meet a negative slice bound), plus walls in pairs (many rejected candidates) and
rectangles whose padded box sticks out over the low edge: its slice wraps, comes out empty, and the reference's check is vacuous there.  The reference never returns
when a map ends up with two obstacles on one cell (its outer `while True` repeats the placement on the SAME map): a seed that draws more than CALL_CAP candidates is
given up and the next one is tried, so the seeds kept are those for which the reference terminates."""
import os
import random
import sys

sys.dont_write_bytecode = True
os.environ.setdefault('MPLBACKEND', 'Agg')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                        # noqa: E402  (sys.path of the reference)
from make_metrics_golden import write_npz       # noqa: E402
import numpy as np                              # noqa: E402

sys.path.insert(0, os.path.join(MG.REF, 'diff_gpmp2', 'datasets'))
import obst_generator as OG                     # noqa: E402

CALL_CAP = 4000
RECT, WALL = 0, 1

# name, kind, side, obstacles, (w_min, w_max, h_min / gw_min, h_max / gw_max, start_x, start_y / gap_y, end_x, end_y), patch_size, patch_size_obs
SETS = [
    ('tar_pit32', RECT, 32, 5, (3, 4, 3, 4, 4, 4, 20, 20), 4.0, 0.0),
    ('tar_pit64', RECT, 64, 7, (6, 7, 6, 7, 9, 9, 41, 41), 5.0, 0.0),
    ('forest32', RECT, 32, 23, (1, 2, 1, 2, 0, 0, 31, 31), 3.0, 1.0),
    ('forest64', RECT, 64, 44, (2, 3, 2, 3, 0, 0, 63, 63), 3.0, 3.0),
    ('multi_obs32', RECT, 32, 2, (4, 14, 4, 14, 3, 3, 28, 28), 2.0, 4.0),
    ('multi_obs64', RECT, 64, 4, (8, 18, 8, 18, 6, 6, 57, 57), 3.0, 6.0),
    ('passage32', WALL, 32, 1, (6, 16, 4, 5, 4, 0, 0, 0), 3.0, 0.0),
    ('passage64', WALL, 64, 1, (12, 22, 4, 5, 9, 0, 0, 0), 3.0, 0.0),
    ('walls64', WALL, 64, 2, (12, 22, 7, 9, 9, 3, 0, 0), 4.0, 0.0),
    ('walls32', WALL, 32, 2, (3, 6, 2, 5, 1, 0, 0, 0), 2.0, 0.0),
    # padded boxes over the low edge: large separations against centres that start at the edge
    ('wrap32', RECT, 32, 6, (2, 5, 2, 5, 0, 0, 31, 31), 5.0, 7.0),
    ('wrap64', RECT, 64, 9, (4, 9, 3, 8, 0, 0, 40, 63), 4.0, 12.0),
]
REPEATS = {'passage32': 12, 'passage64': 12, 'walls64': 6, 'walls32': 6, 'wrap32': 4, 'wrap64': 3}


class GaveUp(Exception):
  pass


def run_reference(kind, side, n, p, patch_size, patch_size_obs, start_pts, goal_pts, seed):
  """-> (candidates (K, 4), map) or None where the reference does not terminate"""
  rec = []
  rect, wall = OG.random_rect, OG.random_wall

  def rec_rect(*a, **kw):
    if len(rec) >= CALL_CAP: raise GaveUp()
    o = rect(*a, **kw)
    rec.append((o.width, o.height, o.center_x, o.center_y))
    return o

  def rec_wall(*a, **kw):
    if len(rec) >= CALL_CAP: raise GaveUp()
    o = wall(*a, **kw)
    rec.append((o.width, o.gap_width, o.center_x, o.gap_y))
    return o
  OG.random_rect, OG.random_wall = rec_rect, rec_wall
  try:
    random.seed(seed)
    if kind == RECT:
      m = OG.generate_rect_obstacle_map((side, side), n, start_pts, goal_pts, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], patch_size=patch_size,
                                        patch_size_obs=patch_size_obs)
    else:
      m = OG.generate_wall_obstacle_map((side, side), n, start_pts, goal_pts, p[0], p[1], p[2], p[3], p[4], p[5], patch_size=patch_size)
  except GaveUp:
    return None
  finally:
    OG.random_rect, OG.random_wall = rect, wall
  return np.asarray(rec, np.int64), m


def main():
  out, names = {}, []
  total = 0
  for si, (name, kind, side, n, p, patch_size, patch_size_obs) in enumerate(SETS):
    for rep in range(REPEATS.get(name, 2)):
      for with_pts in (False, True):
        rs = np.random.RandomState(1100 + 10 * si + rep)
        start_pts = goal_pts = None
        if with_pts:      # pixel coordinates (x, y) with fractions; the second start point sits near the low edges
          start_pts = rs.uniform(2.0, side - 3.0, (2, 2))
          goal_pts = rs.uniform(2.0, side - 3.0, (2, 2))
          start_pts[1] = rs.uniform(0.05, 1.6, 2)
        seed = 5000 + 100 * si + 10 * rep
        while True:
          r = run_reference(kind, side, n, p, patch_size, patch_size_obs, start_pts, goal_pts, seed)
          if r is not None: break
          seed += 1
        cands, m = r
        assert m.shape == (side, side) and set(np.unique(m)) <= {0.0, 1.0}
        case = '%s_r%d_%s' % (name, rep, 'pts' if with_pts else 'nopts')
        names.append(case)
        out[case + '_params'] = np.asarray([kind, side, n] + list(p), np.int32)
        out[case + '_patch'] = np.asarray([patch_size, patch_size_obs], np.float64)
        out[case + '_cands'] = cands.astype(np.int32)
        out[case + '_map'] = m.astype(np.uint8)
        out[case + '_seed'] = np.int64(seed)
        if with_pts:
          out[case + '_start_pts'], out[case + '_goal_pts'] = start_pts, goal_pts
        total += len(cands)
        print('%-26s seed %d: %3d candidates for %2d obstacles, %4d obstacle cells' % (case, seed, len(cands), n, int((m == 0).sum())))
  out['cases'] = np.array(names)
  path = os.path.join(HERE, 'g11_obstacles.npz')
  write_npz(path, out)
  print('wrote g11_obstacles.npz %.1f KB, %d cases, %d candidates' % (os.path.getsize(path) / 1024.0, len(names), total))


if __name__ == '__main__':
  main()
