#!/usr/bin/env python
"""Generate tests/golden/g9_metrics.npz: the validation metrics of the reference's test loop (learning/test_planner.py:299-334) on small batches of
trajectories, computed by the REAL reference the way that loop calls it -- one trajectory at a time:
  smoothness_metrics / collision_metrics (utils/planner_utils.py:75-102), GPFactor.get_error, ObstacleFactor(state_dim, steps, 0.0, env, robot).get_error
  (test_planner.py:139-140, :300-304), torch.nn.MSELoss against the expert trajectory (:342-344) and the velocity-limit loop (:310-322).
Only arrays are stored.  Re-run with:   python tests/golden/make_metrics_golden.py   (the file regenerates byte for byte: fixed seeds, fixed zip timestamps)

make_golden.py (imported for its two in-process shims -- the tolerant plt.style.use and Tensor.byte -> bool -- and for where the reference lives) is left as it is.

Two things the reference cannot do as called, and what is done instead:
  * ObstacleFactor's batched get_error with a Python-float eps and the robot's 1-D radius vector: obstacle_cost.py:30-33 reshapes `eps + r_vec` as a
    three-dimensional tensor.  The SAME value is passed as a (1, n, 1, 1) tensor (what obsfactor.set_eps does at test_planner.py:182-184, with zeros).
  * d = 6: PointRobotXYH has no batched sphere model, so the obstacle errors come from the unbatched pieces, HingeLossObstacleCost.hinge_loss_signed_batch
    on state[0:2], as make_golden.py does for g3_c4_xyh.

Columns of <case>_metrics (B, 13): include/dgpmp2_hip.h, DGP_METRIC_*.  num_penetrating holds the plain COUNT of penetrating interior states; the reference's own
`numel / 2` (1.5 x that, it is called with an (n,1,1) tensor) is kept as <case>_ref_num_penetrating, and coll_intensity is the reference's value as it stands."""
import io
import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG      # noqa: E402  (shims, sys.path of the reference, float64 default)
import numpy as np            # noqa: E402
import torch                  # noqa: E402
from diff_gpmp2.gpmp2.gp import GPFactor                                              # noqa: E402
from diff_gpmp2.gpmp2.obstacle import ObstacleFactor                                  # noqa: E402
from diff_gpmp2.gpmp2.obstacle.obstacle_cost import HingeLossObstacleCost             # noqa: E402
from diff_gpmp2.robot_models import PointRobot2D                                      # noqa: E402
from diff_gpmp2.utils.planner_utils import smoothness_metrics, collision_metrics      # noqa: E402
from oracle.gpmp2_oracle import circles_sdf, C2_CIRCLES, straight_line_trajb, bilinear_interpolate      # noqa: E402

NAMES = ('avg_vel', 'avg_acc', 'avg_jerk', 'gp_mse', 'in_coll', 'num_penetrating', 'avg_penetration', 'max_penetration', 'coll_intensity',
         'constraint_violation', 'pos_mse', 'vel_mse', 'traj_mse')
T_SEC, RADIUS, V_LIM = 10.0, 0.4, 1.0
MARGIN = 1e-9
# (name, dof, n, B, grid side, crop (H, W) or None, metric_eps, velocity limits)
CASES = (('c0', 2, 4, 6, 64, None, 0.0, False),
         ('c1', 2, 33, 8, 64, None, 0.4, True),
         ('c2', 2, 64, 8, 128, None, 0.0, True),
         ('c3', 2, 101, 6, 48, (40, 48), 0.4, False),      # non-square: the 48-cell grid cropped to its first 40 rows (res = 10 / 48)
         ('c4', 3, 64, 6, 64, None, 0.0, True))
# start / goal positions by kind: collision-free, deeply penetrating (through the circles' centres), leaving the grid, outside it altogether
ENDS = {'free': ((-4.5, 4.0), (4.5, 4.2)), 'deep': ((-4.0, -1.0), (3.0, 0.2)), 'deep2': ((-2.0, -3.0), (1.5, 3.5)), 'leave': ((3.0, -4.0), (7.5, -4.5)),
        'outside': ((6.0, 6.0), (8.0, -6.0)), 'free2': ((-4.6, -4.5), (4.0, -4.2)), 'graze': ((-4.0, 1.2), (4.0, -2.2)), 'leave_y': ((-3.0, 3.0), (-3.5, 6.5))}
KINDS = ('free', 'deep', 'leave', 'deep2', 'outside', 'graze', 'free2', 'leave_y')


def f32(a): return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)      # every input is an fp32 number: fp32 and fp64 I/O see the same values


def grid_of(G, crop):
  sdf = circles_sdf(G, C2_CIRCLES)
  if crop is not None: sdf = sdf[:crop[0], :crop[1]]
  return np.ascontiguousarray(sdf)[None, None]


def trajectories(rs, dof, n, B, vel):
  d = 2 * dof
  start, goal = np.zeros((B, 1, d)), np.zeros((B, 1, d))
  for b in range(B):
    s, g = ENDS[KINDS[b % len(KINDS)]]
    start[b, 0, :2], goal[b, 0, :2] = s, g
  if dof == 3: goal[:, 0, 2] = rs.uniform(-np.pi, np.pi, B)
  th = straight_line_trajb(start[:, :, :dof], goal[:, :, :dof], T_SEC, n - 1, dof) + rs.randn(B, n, d) * 0.05
  if vel:      # columns 2 and 3 (d = 6: theta and v_x -- the reference's loop reads s[2], s[3] whatever dof): odd trajectories break the limit at every third state
    v = np.clip(th[:, :, 2:4], -0.9, 0.9)
    fast = ((np.arange(n)[None, :] + np.arange(B)[:, None]) % 3 == 0) & (np.arange(B)[:, None] % 2 == 1)
    v[fast] = np.where(rs.rand(int(fast.sum()), 2) < 0.5, -1.0, 1.0) * rs.uniform(1.2, 2.0, (int(fast.sum()), 2))
    v[fast & (np.arange(n)[None, :] % 2 == 0), 1] *= 0.3      # only one of the two columns beyond its limit
    th[:, :, 2:4] = v
  th_opt = th + rs.randn(B, n, d) * 0.1
  return f32(th), f32(th_opt)


def reference_metrics(dof, n, th, th_opt, sdf, eps, vel):
  """one trajectory at a time, as learning/test_planner.py:299-334 does -> (metrics (B, 13), ref_num_penetrating (B), obs_error (B, n))"""
  B, steps, d = th.shape[0], n - 1, 2 * dof
  dt = T_SEC * 1.0 / steps * 1.0
  gpfactor = GPFactor(dof, dt, steps)
  robot = PointRobot2D(torch.tensor(RADIUS), 1, n)
  obsfactor = ObstacleFactor(d, steps, 0.0, MG.ENV, robot)
  hinge = HingeLossObstacleCost(MG.ENV)
  eps_traj = torch.full((1, n, 1, 1), float(eps))      # the Python-float eps as the tensor the batched path needs (see the module docstring)
  obsfactor.set_eps(eps_traj)
  criterion = torch.nn.MSELoss()
  sdf_t = MG.T(sdf)
  M, ref_num, oerr = np.zeros((B, len(NAMES))), np.zeros(B), np.zeros((B, n))
  for b in range(B):
    th_final, opt = MG.T(th[b:b + 1]), MG.T(th_opt[b])
    avg_vel, avg_acc, avg_jerk = smoothness_metrics(th_final[0], T_SEC, steps)
    gp_error, _, _ = gpfactor.get_error(th_final)
    if dof == 2: obs_error, _ = obsfactor.get_error(th_final, sdf_t)
    else: obs_error, _ = hinge.hinge_loss_signed_batch(th_final[:, :, 0:2].reshape(1, n, 1, 2), torch.tensor(RADIUS), eps_traj, sdf_t)
    assert tuple(obs_error[0].shape) == (n, 1, 1) and tuple(gp_error.shape) == (1, steps, d, 1)
    mse_gp = torch.mean(torch.sum(gp_error ** 2, dim=-1))
    in_coll, avg_pen, max_pen, coll_int = collision_metrics(th_final[0], obs_error[0], T_SEC, steps)
    violation = 0.0
    if vel:
      for i in range(th_final.shape[1]):
        s = th_final[0][i]
        if not (torch.abs(s[2]) <= V_LIM and torch.abs(s[3]) <= V_LIM): violation += 1.0
    violation = violation / (th_final.shape[1] * 1.0)
    count = int(torch.count_nonzero(obs_error[0][1:-1]))
    ref_num[b] = torch.numel(torch.nonzero(obs_error[0][1:-1, :])) / 2
    assert ref_num[b] == 1.5 * count and bool(in_coll) == (count > 0)      # the three-column nonzero() of the (n-2,1,1) tensor
    M[b] = (avg_vel.item(), avg_acc.item(), avg_jerk.item(), mse_gp.item(), float(bool(in_coll)), float(count), avg_pen.item(), max_pen.item(), float(coll_int),
            violation, criterion(th_final[0][:, 0:dof], opt[:, 0:dof]).item(), criterion(th_final[0][:, dof:], opt[:, dof:]).item(), criterion(th_final[0], opt).item())
    oerr[b] = MG.N(obs_error[0]).reshape(n)
  return M, ref_num, oerr


def decidable(th, sdf, eps, vel, G_cols):
  """no state within MARGIN of the hinge threshold, no velocity within MARGIN of its limit: the counts do not hang on a rounding"""
  B, n = th.shape[:2]
  dist, _ = bilinear_interpolate(np.broadcast_to(sdf[:, 0], (B,) + sdf.shape[-2:]), th[:, :, :2], 10.0 / G_cols, MG.ENV['x_lims'], MG.ENV['y_lims'])
  assert np.min(np.abs(dist - (eps + RADIUS))) > MARGIN, 'a state lies on the hinge threshold'
  if vel: assert np.min(np.abs(np.abs(th[:, :, 2:4]) - V_LIM)) > MARGIN, 'a velocity lies on its limit'


def write_npz(path, arrays):
  """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes"""
  with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
    for k in sorted(arrays):
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
      info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      z.writestr(info, buf.getvalue())


def main():
  out = {'names': np.array(NAMES), 'cases': np.array([c[0] for c in CASES] + ['tie']), 'circles': np.asarray(C2_CIRCLES), 'total_time_sec': T_SEC, 'radius': RADIUS,
         'v_lim': V_LIM}
  for k, (name, dof, n, B, G, crop, eps, vel) in enumerate(CASES):
    rs = np.random.RandomState(900 + k)
    th, th_opt = trajectories(rs, dof, n, B, vel)
    sdf = grid_of(G, crop)
    decidable(th, sdf, eps, vel, sdf.shape[-1])
    M, ref_num, oerr = reference_metrics(dof, n, th, th_opt, sdf, eps, vel)
    assert M[:, 4].min() == 0.0 and M[:, 4].max() == 1.0, 'a case must hold colliding and collision-free trajectories'
    if vel: assert (M[:, 9] > 0).any() and (M[:, 9] == 0).any()
    for key, v in (('dof', dof), ('n', n), ('G', G), ('hw', sdf.shape[-2:]), ('eps', eps), ('vel', int(vel)), ('th', th), ('th_opt', th_opt), ('metrics', M),
                   ('ref_num_penetrating', ref_num), ('obs_error', oerr)):
      out['%s_%s' % (name, key)] = np.asarray(v)
    print('%s: dof %d n %3d B %d grid %s eps %.1f vel %d  in_coll %s  count %s' % (name, dof, n, B, tuple(sdf.shape[-2:]), eps, vel, M[:, 4].astype(int), M[:, 5].astype(int)))
  # the exact tie, built like fixture G1's Q5 tie (make_golden.py:118-122): a constant grid equal to eps + r.  dist <= eps + r holds with equality wherever the
  # bilinear weights reproduce the constant exactly; the error there is 0.0 (not counted), a state whose interpolated distance rounds just below has a tiny positive one
  dof, n, B, eps = 2, 16, 4, 0.4
  rs = np.random.RandomState(990)
  th, th_opt = trajectories(rs, dof, n, B, False)
  sdf = np.full((1, 1, 16, 16), eps + RADIUS)
  M, ref_num, oerr = reference_metrics(dof, n, th, th_opt, sdf, eps, False)
  dist, _ = bilinear_interpolate(np.broadcast_to(sdf[:, 0], (B, 16, 16)), th[:, :, :2], 10.0 / 16, MG.ENV['x_lims'], MG.ENV['y_lims'])
  assert (dist.reshape(B, n)[:, 1:-1] == eps + RADIUS).any(), 'no exact tie among the interior states'
  for key, v in (('dof', dof), ('n', n), ('G', 16), ('hw', (16, 16)), ('eps', eps), ('vel', 0), ('th', th), ('th_opt', th_opt), ('metrics', M), ('ref_num_penetrating', ref_num),
                 ('obs_error', oerr), ('const', eps + RADIUS)):
    out['tie_%s' % key] = np.asarray(v)
  print('tie: exact ties at %d of %d interior states, count %s' % (int((dist.reshape(B, n)[:, 1:-1] == eps + RADIUS).sum()), B * (n - 2), M[:, 5].astype(int)))
  path = os.path.join(HERE, 'g9_metrics.npz')
  write_npz(path, out)
  print('wrote g9_metrics.npz %.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
  main()
