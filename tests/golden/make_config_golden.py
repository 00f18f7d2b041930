#!/usr/bin/env python
"""Generate tests/golden/g11_config_constants.npz: the REAL reference run AWAY from the constants every other fixture was recorded at -- parity_cases.ND
(total_time_sec 7, K_s 0.02, K_g 0.005, cost_sigma 0.03, epsilon_dist 0.25, radius 0.3, reg 0.05, x_lims (-3, 8), y_lims (-4, 6)) with Q_c_inv = 2.5 I, K_v 0.02,
v_x 0.6, v_y 0.9, K_d 0.05 -- on the inputs of parity_cases.nondefault_inputs (B = 4, n = 13, one 33 x 37 grid), and, for the problem sampler's oracle, Env2D at
x_lims (-3, 7), y_lims (-6, 2) on 26 x 20 grids with total_time_sec 7.
Only arrays are stored.  Re-run with:   python tests/golden/make_config_golden.py   (the file regenerates byte for byte: fixed seeds, fixed zip timestamps)

make_golden.py, make_metrics_golden.py and make_problems_golden.py (imported for their shims, for where the reference lives and for their helpers) are left as they are.

  (a) PlanLayer.forward, dof 2, three ways: static covariances (`static_*`), the velocity-limit factor (`vel_*`: the reference's batched path cannot run it, SURVEY a9,
      so one trajectory at a time from its unbatched factor as g3_c3_vel does) and per-state qc / ow / eps tensors (`cov_*`)
  (b) dof 3 with the non-holonomic factor (`xyh_*`), built as g3_c4_xyh builds it
  (c) autograd of sum(gbar dtheta) (`g_*`) and of sum(gext err_ext) (`ge_*`) w.r.t. th, sdf, start, goal, qc, ow, eps, as g5_grads records them
  (d) the three unweighted errors at th (`unw_*`)
  (e) smoothness_metrics / collision_metrics and the velocity-limit loop of learning/test_planner.py:310-322 with v_x != v_y (`met_*`)
  (f) Env2D.get_signed_obstacle_distance / is_feasible (`env_*`) and straight_line_trajb (`line_*`) for the sampler's oracle"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                        # noqa: E402  (shims, sys.path of the reference, float64 default)
import make_metrics_golden as MM                # noqa: E402
import make_problems_golden as MP               # noqa: E402
import numpy as np                              # noqa: E402
import torch                                    # noqa: E402
sys.path.insert(0, os.path.join(MG.ROOT, 'tests'))
import parity_cases as PC                       # noqa: E402  (the inputs' builder, shared with the tests)
import problems_cases as PCS                    # noqa: E402
from diff_gpmp2.env.env_2d import Env2D                                                 # noqa: E402
from diff_gpmp2.gpmp2.diff_gpmp2_planner import DiffGPMP2Planner                        # noqa: E402
from diff_gpmp2.gpmp2.plan_layer import PlanLayer                                       # noqa: E402
from diff_gpmp2.robot_models import PointRobot2D                                        # noqa: E402
from diff_gpmp2.utils.planner_utils import straight_line_trajb                          # noqa: E402

T, N = MG.T, MG.N
ND = PC.ND
ENV = {'x_lims': list(ND['x_lims']), 'y_lims': list(ND['y_lims'])}
B_, N_ = 4, 13


def dicts(dof, n, **plp_extra):
  t = lambda v: torch.tensor(float(v))
  gp = {'Q_c_inv': 2.5 * torch.eye(dof), 'K_s': t(ND['K_s']), 'K_g': t(ND['K_g']), 'K_v': t(PC.ND_VEL['K_v']), 'v_x': [PC.ND_VEL['v_x']], 'v_y': [PC.ND_VEL['v_y']],
        'K_d': t(PC.ND_DYN['K_d'])}
  obs = {'cost_sigma': t(ND['cost_sigma']), 'epsilon_dist': t(ND['epsilon_dist'])}
  plp = dict({'dof': dof, 'state_dim': 2 * dof, 'total_time_sec': ND['total_time_sec'], 'total_time_step': n - 1}, **plp_extra)
  opt = {'method': 'gauss_newton', 'reg': ND['reg'], 'plan_time': float('inf'), 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  return gp, obs, plp, opt


def forward_rows(out):
  B, n = B_, N_
  x = PC.nondefault_inputs(2, n, B, 'perstate', 'f32')
  gp, obs, plp, opt = dicts(2, n)
  planner = DiffGPMP2Planner(gp, obs, plp, opt, ENV, PointRobot2D(torch.tensor(ND['radius']), B, n), batch_size=B)
  sdf = T(np.repeat(x.sdf, B, 0))
  im = (sdf > 0).double()
  p = PC.nd_params(2, n, Q_c_inv=2.5 * np.eye(2))
  sq, so, se = p.static_covs(B)
  qc, ow, eps = T(x.qc), T(x.ow.reshape(B, n, 1, 1)), T(x.eps.reshape(B, n, 1, 1))
  gen = torch.Generator().manual_seed(111)
  gbar, gext = T(PC.rnd(torch.randn(B, n, 4, generator=gen).numpy(), 'f32')), T(PC.rnd(torch.randn(B, 1, 1, generator=gen).numpy(), 'f32'))
  out.update(n=n, Q_c_inv=2.5 * np.eye(2), th=x.th, start=x.start, goal=x.goal, sdf=x.sdf, qc=qc, ow=ow, eps=eps, gbar=gbar, gext=gext)
  # (a) static covariances, (d) the unweighted errors at th with the epsilons that forward left behind
  dth, err, eex = planner.plan_layer(T(x.th), T(x.start), T(x.goal), im, sdf, T(sq), T(so), T(se))
  usg, ugp, uob = planner.unweighted_errors_batch(T(x.th), sdf)
  out.update(static_dth=dth, static_err=err, static_errext=eex, unw_sg=usg, unw_gp=ugp, unw_obs=uob)
  # (a) per-state tensors and (c) the gradients
  leaves = [v.clone().requires_grad_(True) for v in (T(x.th), sdf, T(x.start), T(x.goal), qc, ow, eps)]
  dth, err, eex = planner.plan_layer(leaves[0], leaves[2], leaves[3], im, leaves[1], leaves[4], leaves[5], leaves[6])
  out.update(cov_dth=dth, cov_err=err, cov_errext=eex, err_requires_grad=bool(err.requires_grad))
  grads = torch.autograd.grad((gbar * dth).sum(), leaves, retain_graph=True, allow_unused=True)
  grads_e = torch.autograd.grad((gext * eex).sum(), leaves, allow_unused=True)
  z = lambda gr, v: torch.zeros_like(v) if gr is None else gr
  for nm, gr, ge, v in zip(('th', 'sdf', 'start', 'goal', 'qc', 'ow', 'eps'), grads, grads_e, leaves):
    out['g_' + nm] = z(gr, v); out['ge_' + nm] = z(ge, v); out['ge_none_' + nm] = ge is None
  # (a) the velocity-limit factor, one trajectory at a time (make_golden.g3_c3_vel)
  import diff_gpmp2.gpmp2.plan_layer as plmod
  plmod.VelocityLimitFactor = MG._patched_vel_factor_cls()
  gp, obs, plp, opt = dicts(2, n, use_vel_limits=True)
  pl = PlanLayer(gp, obs, plp, opt, ENV, PointRobot2D(torch.tensor(ND['radius']), 1, n), None, 1, False)
  qc1, ow1, eps1 = T(sq[:1]), T(so[:1]), T(se[:1])
  dths, errs = [], []
  for i in range(B):
    t1 = T(x.th[i:i + 1])
    pl.start_prior.set_mean(T(x.start[i:i + 1])); pl.goal_prior.set_mean(T(x.goal[i:i + 1]))
    pl.gp_prior.set_Q_c_inv(qc1); pl.obs_factor.set_inv_cov(ow1); pl.obs_factor.set_eps(eps1)
    eo = pl.obs_factor.get_error(t1, T(x.sdf))
    c_v, H_v = pl.vel_factor.get_error_full(t1[0])
    A, b, K = MG._dense_from_ref(pl, t1, None, None, eo, c_v, H_v, pl.vel_factor.get_inv_cov_full(), 'vel')
    dths.append(pl.solve_linear_system_batch(A, b, K, delta=ND['reg']))
    errs.append(0.5 * torch.bmm(torch.bmm(b.transpose(1, 2), K), b) / pl.M)
  out.update(vel_dth=torch.cat(dths, 0), vel_err=torch.cat(errs, 0), vel_M=pl.M)
  assert (np.abs(x.th[:, :, 2]) >= PC.ND_VEL['v_x']).any() and (np.abs(x.th[:, :, 3]) >= PC.ND_VEL['v_y']).any() and (np.abs(x.th[:, :, 2:]) < PC.ND_VEL['v_x']).any()


def xyh_rows(out):
  """(b): make_golden.g3_c4_xyh at ND"""
  from diff_gpmp2.gpmp2.obstacle.obstacle_cost import HingeLossObstacleCost
  B, n = B_, N_
  x = PC.nondefault_inputs(3, n, B, 'static', 'f32')
  gp, obs, plp, opt = dicts(3, n, non_holonomic=True)

  class _XYH(object):
    nlinks = 1
    def get_sphere_radii(self): return torch.tensor(ND['radius'])
  pl = PlanLayer(gp, obs, plp, opt, ENV, _XYH(), None, 1, False)
  hl = HingeLossObstacleCost(ENV)
  p = PC.nd_params(3, n, Q_c_inv=2.5 * np.eye(3))
  sq, so, se = p.static_covs(1)
  H_fk = torch.zeros(2, 6); H_fk[0, 0] = 1; H_fk[1, 1] = 1
  dths, errs = [], []
  for i in range(B):
    t1 = T(x.th[i:i + 1])
    pl.start_prior.set_mean(T(x.start[i:i + 1])); pl.goal_prior.set_mean(T(x.goal[i:i + 1]))
    pl.gp_prior.set_Q_c_inv(T(sq)); pl.obs_factor.set_inv_cov(T(so))
    e_o, H_e = hl.hinge_loss_signed_batch(t1[:, :, 0:2].reshape(1, n, 1, 2), torch.tensor(ND['radius']), T(se), T(x.sdf))
    H_o = torch.einsum('bsij,jk->bsik', H_e, H_fk)
    e_d, H_d = pl.dyn_factor.get_error_full(t1[0])
    A, b, K = MG._dense_from_ref(pl, t1, None, None, (e_o, H_o), e_d, H_d, pl.dyn_factor.get_inv_cov_full(), 'dyn')
    dths.append(pl.solve_linear_system_batch(A, b, K, delta=ND['reg']))
    errs.append(0.5 * torch.bmm(torch.bmm(b.transpose(1, 2), K), b) / pl.M)
  out.update(xyh_Q_c_inv=2.5 * np.eye(3), xyh_th=x.th, xyh_start=x.start, xyh_goal=x.goal, xyh_dth=torch.cat(dths, 0), xyh_err=torch.cat(errs, 0), xyh_M=pl.M)


MET_EPS = 0.1
MET_FREE = np.array([[-2.5, -3.5, -2.0, 1.5], [-2.5, -3.0, 2.5, -3.2]])      # collision-free; |v_y| between the two limits and |v_x| below both / |v_x| between them


def metrics_inputs():
  """the four trajectories of the forward rows and two collision-free ones, an expert trajectory each -> th, th_opt (6, 13, 4)"""
  n = N_
  x = PC.nondefault_inputs(2, n, B_, 'static', 'f32')
  rs = np.random.RandomState(112)
  s, g = np.zeros((2, 1, 2)), np.zeros((2, 1, 2))
  s[:, 0], g[:, 0] = MET_FREE[:, :2], MET_FREE[:, 2:]
  free = MM.straight_line_trajb(s, g, ND['total_time_sec'], n - 1, 2) + rs.randn(2, n, 4) * 0.02
  th = MM.f32(np.concatenate([x.th, free]))
  return th, MM.f32(th + rs.randn(*th.shape) * 0.1), x.sdf


def metrics_rows(out):
  """(e): make_metrics_golden.reference_metrics with the module constants it reads set to ND, and the velocity-limit loop with its two limits"""
  th, th_opt, sdf = metrics_inputs()
  saved = (MM.T_SEC, MM.RADIUS, MG.ENV)
  MM.T_SEC, MM.RADIUS, MG.ENV = ND['total_time_sec'], ND['radius'], ENV
  try:
    M, ref_num, oerr = MM.reference_metrics(2, N_, th, th_opt, sdf, MET_EPS, False)
  finally:
    MM.T_SEC, MM.RADIUS, MG.ENV = saved
  vx, vy = PC.ND_VEL['v_x'], PC.ND_VEL['v_y']
  for b in range(th.shape[0]):      # learning/test_planner.py:310-322
    violation = 0.0
    for i in range(th.shape[1]):
      s = T(th[b, i])
      if torch.abs(s[2]) <= vx and torch.abs(s[3]) <= vy: continue
      violation = violation + 1.0
    M[b, MM.NAMES.index('constraint_violation')] = violation / (th.shape[1] * 1.0)
  cv = M[:, MM.NAMES.index('constraint_violation')]
  swapped = np.mean(~((np.abs(th[:, :, 2]) <= vy) & (np.abs(th[:, :, 3]) <= vx)), axis=1)
  assert (cv != swapped).sum() >= 2 and M[:, 4].min() == 0.0 and M[:, 4].max() == 1.0, (cv, swapped, M[:, 4])
  dist = MM.bilinear_interpolate(np.broadcast_to(sdf[:, 0], (th.shape[0],) + sdf.shape[-2:]), th[:, :, :2], (ENV['x_lims'][1] - ENV['x_lims'][0]) / sdf.shape[-1], ENV['x_lims'], ENV['y_lims'])[0]
  assert np.min(np.abs(dist - (MET_EPS + ND['radius']))) > MM.MARGIN and np.min(np.abs(np.abs(th[:, :, 2]) - vx)) > MM.MARGIN and np.min(np.abs(np.abs(th[:, :, 3]) - vy)) > MM.MARGIN
  out.update(met_th=th, met_th_opt=th_opt, met_eps=MET_EPS, met_metrics=M, met_ref_num_penetrating=ref_num, met_obs_error=oerr, met_names=np.array(MM.NAMES))


def env_points(H, W, rs):
  """points for Env2D at PCS.ND_X / ND_Y: pixel corners and centres of the box, the closed limit edges, just outside each of the four limits, the last column and
  the row the lower limit falls on, random interior points"""
  (x0, x1), (y0, y1) = PCS.ND_X, PCS.ND_Y
  res = (x1 - x0) / W
  pts = []
  for j in (0, 1, W // 2, W - 2, W - 1):
    for i in (0, 1, 5, 14, 15):
      pts.append((x0 + j * res, y1 - i * res)); pts.append((x0 + (j + 0.5) * res, y1 - (i + 0.5) * res))
  for t in np.linspace(0.0, 1.0, 9):
    pts.append((x1 - t * res, rs.uniform(y0 + 0.1, y1 - 0.1)))      # last column, px in [W - 1, W]
    pts.append((rs.uniform(x0 + 0.1, x1 - 0.1), y0 + t * res))      # the rows at the lower limit: py in [H - 3, H - 2]
    pts.append((x0, y0 + t * (y1 - y0))); pts.append((x1, y0 + t * (y1 - y0))); pts.append((x0 + t * (x1 - x0), y0)); pts.append((x0 + t * (x1 - x0), y1))      # the closed edges
  e = 1e-7
  pts += [(x0 - e, -1.0), (x1 + e, -1.0), (1.0, y0 - e), (1.0, y1 + e), (-4.0, 0.0), (7.5, -3.0), (0.0, 2.5), (0.0, -6.5), (-5.0, -5.0), (5.0, 5.0), (2.5, 4.0), (1e6, 1e6)]
  pts += [(-3.0, 2.0 + e), (7.0, -6.0 - e), (6.9, 1.9), (-2.9, -5.9)]      # symmetric-limit mistakes: inside (-5, 5)^2 but outside these limits, and the reverse
  pts += [(rs.uniform(x0, x1), rs.uniform(y0, y1)) for _ in range(40)]
  return np.asarray(pts, np.float64)


def sampler_rows(out):
  H, W = PCS.ND_HW
  env_params = {'x_lims': list(PCS.ND_X), 'y_lims': list(PCS.ND_Y)}
  f = PCS.fields_nd()
  fields = {'circles': PC.rnd(PC.nd_grid(H, W, PCS.ND_X, PCS.ND_Y, ((0.0, -1.0, 1.2), (4.5, -4.0, 1.0), (5.5, 0.5, 0.8)))[0, 0], 'f32'), 'corners': f[PCS.CORNERS], 'clutter': f[PCS.CLUTTER]}
  out['env_fields'] = np.array(sorted(fields)); out['env_clearance'] = PCS.CLEARANCE
  for k, name in enumerate(sorted(fields)):
    sdf = np.ascontiguousarray(fields[name])
    env = Env2D(env_params)
    env.initialize_from_image(np.ones((H, W)), sdf)
    pts = env_points(H, W, np.random.RandomState(1100 + k))
    with MP.uint8_comparisons():
      dist = np.array([float(env.get_signed_obstacle_distance(T(q).reshape(1, 1, 2))[0].item()) for q in pts])
      verdict = np.array([bool(env.is_feasible(T(q), PCS.CLEARANCE)) for q in pts])
    inside = (pts[:, 0] >= PCS.ND_X[0]) & (pts[:, 0] <= PCS.ND_X[1]) & (pts[:, 1] >= PCS.ND_Y[0]) & (pts[:, 1] <= PCS.ND_Y[1])
    max_d = PCS.ND_X[1] - PCS.ND_X[0]
    assert (dist[~inside] == max_d).all() and (dist[inside] != max_d).all() and (~inside).sum() >= 12, 'MAX_D exactly outside the limits'
    assert verdict[inside].any() and not verdict[inside].all()
    out['env_%s_sdf' % name], out['env_%s_points' % name], out['env_%s_dist' % name], out['env_%s_feasible' % name] = sdf, pts, dist, verdict
    print('%s: %d points, %d inside, %d feasible' % (name, len(pts), int(inside.sum()), int(verdict.sum())))
  rs = np.random.RandomState(1110)
  B = 5
  start, goal = np.zeros((B, 1, 4)), np.zeros((B, 1, 4))
  start[:, 0, 0], goal[:, 0, 0] = rs.uniform(-2.5, 6.5, B), rs.uniform(-2.5, 6.5, B)
  start[:, 0, 1], goal[:, 0, 1] = rs.uniform(-5.5, 1.5, B), rs.uniform(-5.5, 1.5, B)
  out['line_start'], out['line_goal'], out['line_total_time_sec'] = start, goal, PCS.ND_T_SEC
  for n in (3, 16):
    out['line_th_n%d' % n] = N(straight_line_trajb(T(start[:, :, :2]), T(goal[:, :, :2]), PCS.ND_T_SEC, n - 1, 2))


def make_config_golden():
  out = {}
  forward_rows(out); xyh_rows(out); metrics_rows(out); sampler_rows(out)
  path = os.path.join(HERE, 'g11_config_constants.npz')
  MM.write_npz(path, {k: (N(v) if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
  print('wrote g11_config_constants.npz %.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
  make_config_golden()
