#!/usr/bin/env python
"""Generate tests/golden/g10_problems.npz: what the problem sampler (dgp_sample_problems) must agree with, computed by the REAL reference --
  Env2D.initialize_from_image + Env2D.is_feasible (env/env_2d.py:49-62, :86-90 over get_signed_obstacle_distance :119-175) on single points, the way
  get_random_2d_confs calls it (datasets/generate_optimal_paths_gpmp2.py:63-73), and straight_line_trajb (utils/planner_utils.py:47-56).
Only arrays are stored.  Re-run with:   python tests/golden/make_problems_golden.py   (the file regenerates byte for byte: fixed seeds, fixed zip timestamps)

make_golden.py / make_metrics_golden.py (imported for their shims, for where the reference lives and for write_npz) are left as they are.

One more in-process shim, for Env2D only: the reference is written for the torch of its day, where a comparison of tensors gives a uint8 tensor, the SUM of two of
them counts how many hold (`(inlimxu + inlimxl) > 1`, env_2d.py:159-166) and torch.where takes a uint8 condition.  Under torch >= 1.2 the comparisons give bool, the
sum saturates at True and `> 1` is never true: every point would read MAX_D.  While Env2D runs, <=, >=, > of tensors return uint8 and torch.where converts its
condition -- the semantics env_2d.py was written against; nothing of the reference is edited.

Fields: the 24 x 24 union-of-circles field of the other fixtures and the mini dataset's 0_sdf.npy (52 x 52), both over [-5, 5]^2.  Points per field: pixel centres
and corners, the last row and column (where the clamped taps coincide), the limits themselves, points outside the limits, random interior points -- each with
the reference's verdict at the reference's clearance (sphere_radius + epsilon_dist + 0.1, generate_optimal_paths_gpmp2.py:124) -- and points judged at a clearance
5e-13 below and above THEIR OWN distance (the verdict hangs on the last bits of the interpolation)."""
import contextlib
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                        # noqa: E402  (shims, sys.path of the reference, float64 default)
from make_metrics_golden import write_npz       # noqa: E402
import numpy as np                              # noqa: E402
import torch                                    # noqa: E402
from diff_gpmp2.env.env_2d import Env2D                                 # noqa: E402
from diff_gpmp2.utils.planner_utils import straight_line_trajb          # noqa: E402
from oracle.gpmp2_oracle import circles_sdf, C2_CIRCLES                 # noqa: E402

CLEARANCE = 0.4 + 0.4 + 0.1      # robot.get_sphere_radii()[0] + obs_params['epsilon_dist'] + 0.1 with the reference's example configuration
TIE = 5e-13
T_SEC = 10.0


@contextlib.contextmanager
def uint8_comparisons():
  names = ('__le__', '__ge__', '__gt__')
  saved = {k: getattr(torch.Tensor, k) for k in names}
  where = torch.where
  try:
    for k in names: setattr(torch.Tensor, k, (lambda f: lambda a, b: f(a, b).to(torch.uint8))(saved[k]))
    torch.where = lambda c, a, b: where(c.bool(), a, b)
    yield
  finally:
    for k in names: setattr(torch.Tensor, k, saved[k])
    torch.where = where


def points_of(H, W, rs):
  res = 10.0 / W
  pts = []
  for j in (0, 1, W // 2, W - 2, W - 1):                      # pixel corners (px, py integers) and centres (half-integers)
    for i in (0, 1, H // 2, H - 2, H - 1):
      pts.append((-5.0 + j * res, 5.0 - i * res))
      pts.append((-5.0 + (j + 0.5) * res, 5.0 - (i + 0.5) * res))
  for t in np.linspace(0.0, 1.0, 9):                          # last column (px in [W - 1, W]) and last row (py in [H - 1, H]), the limits included
    pts.append((5.0 - t * res, rs.uniform(-4.9, 4.9)))
    pts.append((rs.uniform(-4.9, 4.9), 5.0 - H * res + t * res))
  pts += [(5.0, 5.0), (-5.0, -5.0), (-5.0, 5.0), (5.0, 5.0 - H * res), (5.0, 0.3), (-5.0, 0.3), (0.3, 5.0), (0.3, 5.0 - H * res)]
  pts += [(5.0000001, 0.0), (-5.0000001, 0.0), (0.0, 5.0000001), (0.0, -5.0000001), (7.0, 7.0), (-9.0, 2.0), (2.0, -100.0), (1e6, 1e6)]      # outside: MAX_D
  pts += [(rs.uniform(-5, 5), rs.uniform(-5, 5)) for _ in range(20)]
  return np.asarray(pts, np.float64)


def main():
  fields = {'circles': np.ascontiguousarray(circles_sdf(24, C2_CIRCLES)),
            'mini': np.load(os.path.join(HERE, 'mini_dataset', 'train', 'im_sdf', '0_sdf.npy')).astype(np.float64)}
  out = {'fields': np.array(sorted(fields)), 'clearance': CLEARANCE, 'total_time_sec': T_SEC}
  n_pts = 0
  for k, name in enumerate(sorted(fields)):
    sdf = fields[name]
    H, W = sdf.shape
    rs = np.random.RandomState(1000 + k)
    env = Env2D(MG.ENV)
    env.initialize_from_image(np.ones((H, W)), sdf)
    pts = points_of(H, W, rs)
    tie = np.asarray([(rs.uniform(-4.5, 4.5), rs.uniform(-4.5, 4.5)) for _ in range(12)], np.float64)
    with uint8_comparisons():
      dist = np.array([float(env.get_signed_obstacle_distance(MG.T(p).reshape(1, 1, 2))[0].item()) for p in pts])
      verdict = np.array([bool(env.is_feasible(MG.T(p), CLEARANCE)) for p in pts])
      tie_dist = np.array([float(env.get_signed_obstacle_distance(MG.T(p).reshape(1, 1, 2))[0].item()) for p in tie])
      tie_pts = np.repeat(tie, 2, axis=0)
      tie_clear = np.stack([tie_dist - TIE, tie_dist + TIE], 1).reshape(-1)
      tie_verdict = np.array([bool(env.is_feasible(MG.T(p), float(c))) for p, c in zip(tie_pts, tie_clear)])
    assert (dist[np.abs(pts).max(1) > 5.0] == 10.0).all() and (dist[np.abs(pts).max(1) <= 5.0] != 10.0).all(), 'MAX_D exactly outside the limits'
    assert verdict.any() and not verdict.all()
    assert tie_verdict.reshape(-1, 2)[:, 0].all() and not tie_verdict.reshape(-1, 2)[:, 1].any() and (np.abs(tie_clear - np.repeat(tie_dist, 2)) < 1e-12).all()
    for key, v in (('sdf', sdf), ('points', np.concatenate([pts, tie_pts])), ('clearances', np.concatenate([np.full(len(pts), CLEARANCE), tie_clear])),
                   ('feasible', np.concatenate([verdict, tie_verdict])), ('dist', np.concatenate([dist, np.repeat(tie_dist, 2)]))):
      out['%s_%s' % (name, key)] = np.asarray(v)
    n_pts += len(pts) + len(tie_pts)
    print('%s: %d x %d, %d points (%d feasible), %d tie points' % (name, H, W, len(pts), int(verdict.sum()), len(tie_pts)))
  # straight_line_trajb for a few start / goal pairs
  rs = np.random.RandomState(1010)
  B = 5
  start, goal = np.zeros((B, 1, 4)), np.zeros((B, 1, 4))
  start[:, 0, :2], goal[:, 0, :2] = rs.uniform(-4.5, 4.5, (B, 2)), rs.uniform(-4.5, 4.5, (B, 2))
  start[0, 0, :2], goal[0, 0, :2] = (-4.8, -4.8), (4.8, 4.8)      # diagonal 0
  out['line_start'], out['line_goal'] = start, goal
  for n in (3, 16, 64):
    th = MG.N(straight_line_trajb(MG.T(start[:, :, :2]), MG.T(goal[:, :, :2]), T_SEC, n - 1, 2))      # (configurations in: (B,1,dof))
    assert th.shape == (B, n, 4) and th.dtype == np.float64
    out['line_th_n%d' % n] = th
  path = os.path.join(HERE, 'g10_problems.npz')
  write_npz(path, out)
  print('wrote g10_problems.npz %.1f KB, %d points' % (os.path.getsize(path) / 1024.0, n_pts))


if __name__ == '__main__':
  main()
