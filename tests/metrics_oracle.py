"""numpy fp64 restatement of the validation metrics dgp_traj_metrics computes (include/dgpmp2_hip.h: DGP_METRIC_*), for batches larger than the fixture
tests/golden/g9_metrics.npz, which pins these definitions against the reference itself.  Built on oracle.gpmp2_oracle's bilinear lookup / hinge and GP factor
error.  Reference: learning/test_planner.py:299-334, utils/planner_utils.py:75-102."""
import numpy as np

from oracle import gpmp2_oracle as O

NAMES = ('avg_vel', 'avg_acc', 'avg_jerk', 'gp_mse', 'in_coll', 'num_penetrating', 'avg_penetration', 'max_penetration', 'coll_intensity',
         'constraint_violation', 'pos_mse', 'vel_mse', 'traj_mse')
COL = {k: i for i, k in enumerate(NAMES)}
REAL = [COL[k] for k in NAMES if k not in ('in_coll', 'num_penetrating')]      # the real-valued columns (the other two are compared exactly)


def obs_error(p, th, sdf, eps):
  """(B, n): raw hinge error of every state at epsilon `eps` (ObstacleFactor(..., eps, ...).get_error(th, sdf)[0][:, :, 0, 0]); sdf (B | 1, 1, H, W)"""
  th = np.asarray(th, np.float64)
  B, n = th.shape[:2]
  sdfb = np.broadcast_to(np.asarray(sdf, np.float64), (B,) + tuple(np.shape(sdf)[1:]))
  e, _ = O.obstacle_error(th, sdfb, np.full((B, n, 1, 1), float(eps)), p)
  return e.reshape(B, n)


def _mean_rows(x, reverse):
  """mean over axis 1, summed in state order or (reverse) against it -- the two orders whose spread the tests may quote"""
  x = x[:, ::-1] if reverse else x
  s = np.zeros(x.shape[0])
  for i in range(x.shape[1]): s = s + x[:, i]
  return s / x.shape[1]


def metrics(p, th, sdf, eps=0.0, th_opt=None, reverse=False):
  """-> (M (B, 13) float64 in the order of NAMES, obs_error (B, n)).  p: O.OracleParams (dof, n, total_time_sec, radius, limits, use_vel_limits)."""
  th = np.asarray(th, np.float64)
  B, n, d = th.shape
  dof, steps = p.dof, float(n - 1)
  M = np.zeros((B, len(NAMES)))
  nrm = lambda a: np.sqrt(np.sum(a * a, axis=-1))
  # smoothness_metrics: columns 2.., divisors total_time_step and total_time_step^2
  d1 = th[:, 1:] - th[:, :-1]
  d2 = d1[:, 1:] - d1[:, :-1]
  M[:, COL['avg_vel']] = _mean_rows(nrm(th[:, :, 2:]), reverse)
  M[:, COL['avg_acc']] = _mean_rows(nrm(d1[:, :, 2:] / steps * 1.0), reverse)
  M[:, COL['avg_jerk']] = _mean_rows(nrm(d2[:, :, 2:] / (steps ** 2.0)), reverse)
  # gp_mse: mean of e^2 over the (n - 1) d entries of the GP factor errors
  e_gp = O.gp_factor_error(th, dof, p.dt)[0][..., 0]
  M[:, COL['gp_mse']] = _mean_rows((e_gp ** 2).reshape(B, -1), reverse)
  # collision_metrics over the interior states; the reference's num_penetrating is 1.5 x the count (nonzero of an (n-2,1,1) tensor has three columns)
  oe = obs_error(p, th, sdf, eps)
  inner = oe[:, 1:-1]
  cnt = np.sum(inner != 0.0, axis=1)
  M[:, COL['num_penetrating']] = cnt
  M[:, COL['in_coll']] = (cnt > 0).astype(np.float64)
  M[:, COL['avg_penetration']] = _mean_rows(inner, reverse)
  M[:, COL['max_penetration']] = np.max(inner, axis=1)
  M[:, COL['coll_intensity']] = ((1.5 * cnt) * p.dt) / p.total_time_sec * 1.0
  if p.use_vel_limits:
    bad = ~((np.abs(th[:, :, 2]) <= p.v_x) & (np.abs(th[:, :, 3]) <= p.v_y))
    M[:, COL['constraint_violation']] = np.sum(bad, axis=1) / (n * 1.0)
  if th_opt is not None:
    sq = (th - np.asarray(th_opt, np.float64)) ** 2
    M[:, COL['pos_mse']] = _mean_rows(sq[:, :, :dof].reshape(B, -1), reverse)
    M[:, COL['vel_mse']] = _mean_rows(sq[:, :, dof:].reshape(B, -1), reverse)
    M[:, COL['traj_mse']] = _mean_rows(sq.reshape(B, -1), reverse)
  return M, oe


def load_case(g, name):
  """-> (OracleParams, th, th_opt, sdf (1,1,H,W), eps, expected metrics (B,13), expected obs_error (B,n), the reference's own num_penetrating)"""
  k = lambda s: g['%s_%s' % (name, s)]
  dof, n, vel = int(k('dof')), int(k('n')), bool(int(k('vel')))
  kw = dict(non_holonomic=True) if dof == 3 else {}
  p = O.OracleParams(dof=dof, total_time_sec=float(g['total_time_sec']), total_time_step=n - 1, radius=float(g['radius']), use_vel_limits=vel,
                     v_x=float(g['v_lim']), v_y=float(g['v_lim']), **kw)
  if name == 'tie': sdf = np.full((1, 1, 16, 16), float(k('const')))
  else:
    H, W = [int(v) for v in k('hw')]
    sdf = O.circles_sdf(int(k('G')), [tuple(c) for c in g['circles']])[None, None, :H, :W]
  return p, k('th'), k('th_opt'), np.ascontiguousarray(sdf), float(k('eps')), k('metrics'), k('obs_error'), k('ref_num_penetrating')


def case_names(g): return [str(c) for c in g['cases']]
