"""dgp_traj_metrics on the GPU, through the C-ABI (tests/harness.py's memory helpers) and through the planner.

  * every case of tests/golden/g9_metrics.npz (the reference's own numbers) in fp64 and fp32 I/O: real-valued columns at parity_cases.TOL_ERR['f64'] (the arithmetic is
    fp64 whatever the I/O type; for fp32 I/O the expected values are tests/metrics_oracle.py fed the fp32-rounded inputs, as the parity cases do), in_coll and
    num_penetrating exactly equal, obs_error at TOL_ERR[io] (it is stored in the I/O type);
  * full-GPU lane-mixed batches (tests/lane_mix.py: every wavefront holds colliding, free and out-of-grid trajectories, hinge decisions alternating from state to
    state), B = 4096 and ragged 4099, n in {64, 101, 300}, per trajectory against tests/metrics_oracle.py; outputs independent of the batch position, bit for bit;
  * shared against per-sample grids, tiled against row-major grids and two runs: bit-equal;
  * consistency with dgp_eval_errors at eps = metric_eps (parity_cases.py's bound for the unweighted errors, TOL_ERR x 10);
  * DiffGPMP2Planner.trajectory_metrics after forward() on the mini dataset, and under torch.cuda.graph capture and replay."""
import os

import numpy as np
import pytest
import torch

import harness
import lane_mix as LM
import metrics_oracle as MO
import parity_cases as PC
from conftest import rel_err
from dgpmp2_amd import _capi
from oracle import gpmp2_oracle as O
from metrics_oracle import load_case, case_names

pytestmark = pytest.mark.gpu
EXACT = [MO.COL['in_coll'], MO.COL['num_penetrating']]


@pytest.fixture(scope='module')
def be():
  return harness.Backend('hip')


def run(be, p, th, sdf, eps, th_opt=None, io='f64', tiled=False, want=(True, True)):
  """dgp_traj_metrics -> (metrics (B,13) float64, obs_error (B,n) as float64); sdf (1 | B, 1, H, W)"""
  be._keep = []
  solver = _capi.Solver(harness.config_from_oracle(p, io), api=be.api)
  B, n = th.shape[:2]
  _, th_p = be.to_dev(th, io)
  _, opt_p = be.to_dev(th_opt, io)
  sdf = np.asarray(sdf)
  shared, (H, W) = sdf.shape[0] == 1, sdf.shape[-2:]
  if tiled:
    til = harness.tile_np(sdf)
    _, sp = be.to_dev(til, io)
    arg = solver.sdf_arg(sp, H, W, 0 if shared else til[0].size, layout=_capi.DGP_SDF_TILED4)
  else:
    _, sp = be.to_dev(sdf, io)
    arg = solver.sdf_arg(sp, H, W, 0 if shared else H * W)
  M, M_p = be.empty((B, _capi.DGP_METRIC_COUNT), dtype=np.float64) if want[0] else (None, None)
  oe, oe_p = be.empty((B, n), io) if want[1] else (None, None)
  solver.traj_metrics(B, th_p, arg, eps, opt_p, M_p, oe_p, be.stream())
  return be.to_np(M), be.to_np(oe)


def expected(p, th, sdf, eps, th_opt, io):
  r = lambda a: None if a is None else PC.rnd(a, io)
  return MO.metrics(p, r(th), r(sdf), eps, r(th_opt))


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_fixture_cases(be, golden, io):
  g = golden('g9_metrics')
  tol = PC.TOL_ERR['f64']
  for name in case_names(g):
    p, th, th_opt, sdf, eps, M, oe, _ = load_case(g, name)
    if io == 'f32': M, oe = expected(p, th, sdf, eps, th_opt, io)      # fp64 arithmetic on the fp32-rounded inputs
    got, got_oe = run(be, p, th, sdf, eps, th_opt, io)
    errs = {MO.NAMES[c]: rel_err(got[:, c], M[:, c]) for c in MO.REAL if np.max(np.abs(M[:, c])) > 0}
    print('%s %s: worst %s; obs_error %.3g' % (name, io, max(errs.items(), key=lambda kv: kv[1]), rel_err(got_oe, oe)))
    np.testing.assert_array_equal(got[:, EXACT], M[:, EXACT], err_msg='%s %s in_coll / num_penetrating' % (name, io))
    for c in MO.REAL:
      if np.max(np.abs(M[:, c])) == 0: assert not got[:, c].any(), (name, io, MO.NAMES[c])
      else: assert errs[MO.NAMES[c]] < tol, (name, io, MO.NAMES[c], errs[MO.NAMES[c]])
    assert rel_err(got_oe, oe) < PC.TOL_ERR[io], (name, io, 'obs_error')
    if io == 'f64': np.testing.assert_array_equal(got_oe, oe)          # the lookup's operation order is the reference's: the same bits
    # without the expert trajectories the three MSE columns are exact zeros and nothing else moves; either output alone
    got0, _ = run(be, p, th, sdf, eps, None, io, want=(True, False))
    mse = [MO.COL[k] for k in ('pos_mse', 'vel_mse', 'traj_mse')]
    keep = [c for c in range(13) if c not in mse]
    assert not got0[:, mse].any() and np.array_equal(got0[:, keep], got[:, keep])
    _, oe_only = run(be, p, th, sdf, eps, None, io, want=(False, True))
    assert np.array_equal(oe_only, got_oe)


def mixed_batch(n, seed=0):
  """a lane-mixed batch of at least 4099 trajectories with velocity limits, an expert trajectory per trajectory, and the launch shape the kernel uses for n"""
  lpt, c = (16, 4) if n <= 64 else ((32, 4) if n <= 128 else (64, 5))
  waves = -(-4099 // LM.tpw(lpt))
  bt = LM.make(2, lpt, c, n, 'static', vel=True, waves=waves, seed=seed, nan=False, io='f32')
  assert bt.B >= 4099
  rs = np.random.RandomState(seed + 1)
  # lane_mix's batches are nearly all in collision at this epsilon (the clamped lookups of the leaving / outside trajectories extrapolate to large penetrations):
  # every fourth trajectory becomes a collision-free one, in the corridor above the circles (at least 1.0 from the nearest, threshold 0.7), so that a wavefront of four
  # holds a lane-mixed colliding trajectory, a leaving one, one outside the grid and a free one; the velocity columns keep lane_mix's pattern of limit violations
  free = np.arange(bt.B) % 4 == 3
  k = int(free.sum())
  a = np.stack([rs.uniform(-4.4, -3.0, k), rs.uniform(4.0, 4.4, k)], -1)[:, None]
  b = np.stack([rs.uniform(3.0, 4.4, k), rs.uniform(4.0, 4.4, k)], -1)[:, None]
  w = (np.arange(n) / (n - 1.0))[None, :, None]
  bt.th[free, :, :2] = PC.rnd(a * (1.0 - w) + b * w + rs.randn(k, n, 2) * 0.02, 'f32')
  bt.free = free
  bt.th_opt = PC.rnd(bt.th + rs.randn(*bt.th.shape) * 0.1, 'f32')
  return bt


def check_per_trajectory(bt, tag, got, got_oe, M, oe, io):
  """per trajectory: counts exact, real columns |got - want| <= tol |want| (every one is a mean of non-negative terms), obs_error at TOL_ERR[io] of the trajectory's largest"""
  bad = []
  B = M.shape[0]
  cnt = np.nonzero((got[:, EXACT] != M[:, EXACT]).any(1))[0]
  bad += ['%s %s: in_coll / num_penetrating %s, expected %s' % (tag, LM._where(bt, b), got[b, EXACT], M[b, EXACT]) for b in cnt[:4]]
  tol = PC.TOL_ERR['f64']
  worst = {}
  for c in MO.REAL:
    e = np.abs(got[:, c] - M[:, c]) / np.maximum(np.abs(M[:, c]), 1e-300)
    e[(got[:, c] == M[:, c])] = 0.0
    e[~np.isfinite(got[:, c])] = np.inf
    worst[MO.NAMES[c]] = float(e.max())
    bad += ['%s %s: %s rel err %.3g >= %.1g' % (tag, LM._where(bt, b), MO.NAMES[c], e[b], tol) for b in np.nonzero(~(e < tol))[0][:4]]
  eo = np.abs(got_oe - oe).max(1) / np.maximum(np.abs(oe).max(1), 1e-300)
  eo[(got_oe == oe).all(1)] = 0.0
  bad += ['%s %s: obs_error rel err %.3g' % (tag, LM._where(bt, b), eo[b]) for b in np.nonzero(~(eo < PC.TOL_ERR[io]))[0][:4]]
  print('%s: worst per-trajectory rel err %s; obs_error %.3g' % (tag, max(worst.items(), key=lambda kv: kv[1]), eo.max()))
  assert (M[:B, MO.COL['in_coll']] == 0).any() and (M[:B, MO.COL['in_coll']] == 1).any()
  return bad


@pytest.mark.parametrize('n', [64, 101, 300])
def test_lane_mixed_full_batches(be, n):
  bt = mixed_batch(n)
  eps = bt.p.epsilon_dist                        # the epsilon the batch's hinge decisions were designed around (lane_mix.MARGIN off the threshold)
  bad = []
  for B, io in ((4096, 'f32'), (4099, 'f32'), (4099, 'f64')):
    th, opt = bt.th[:B], bt.th_opt[:B]
    M, oe = expected(bt.p, th, bt.sdf, eps, opt, io)
    got, got_oe = run(be, bt.p, th, bt.sdf, eps, opt, io)
    bad += check_per_trajectory(bt, 'n %d B %d %s' % (n, B, io), got, got_oe, M, oe, io)
    if B == 4099 and io == 'f32':
      # every wavefront mixes kinds: colliding and free trajectories side by side
      T = LM.tpw(bt.lpt)
      assert not M[bt.free[:B], MO.COL['in_coll']].any() and M[~bt.free[:B], MO.COL['in_coll']].mean() > 0.9
      if T > 1:      # (four trajectories per wavefront: every wavefront; two: every other one)
        ic = M[:4096, MO.COL['in_coll']].reshape(-1, T)
        assert ((ic.min(1) == 0) & (ic.max(1) == 1)).mean() > (0.9 if T >= 4 else 0.45)
      # the same trajectories one batch position further on: the same bits (no atomics, a fixed reduction order per trajectory)
      r = 1
      got_r, oe_r = run(be, bt.p, np.roll(th, r, 0), bt.sdf, eps, np.roll(opt, r, 0), io)
      bad += LM.check_bit_equal(bt, 'metrics', got, got_r, r) + LM.check_bit_equal(bt, 'obs_error', got_oe, oe_r, r)
  assert not bad, '\n'.join(bad)


def test_grid_layouts_sharing_and_repeatability_are_bit_equal(be):
  """one arithmetic whatever the grid's layout and ownership: tiled == row-major, shared == the same grid once per trajectory, a second run == the first"""
  rs = np.random.RandomState(5)
  for dof, n, hw in ((2, 64, LM.ODD_GRID), (3, 33, (40, 40))):      # 39 x 41: padding cells in the last tile row and column
    B, d = 1027, 2 * dof
    p = O.OracleParams(dof=dof, total_time_step=n - 1, non_holonomic=dof == 3)
    start, goal = np.zeros((B, 1, d)), np.zeros((B, 1, d))
    start[:, 0, :2], goal[:, 0, :2] = rs.uniform(-5.5, 5.5, (B, 2)), rs.uniform(-5.5, 5.5, (B, 2))
    th = PC.rnd(O.straight_line_trajb(start[:, :, :dof], goal[:, :, :dof], 10.0, n - 1, dof) + rs.randn(B, n, d) * 0.05, 'f32')
    sdf = PC.rnd(O.circles_sdf(max(hw), LM.CIRCLES)[None, None, :hw[0], :hw[1]], 'f32')
    per = np.ascontiguousarray(np.broadcast_to(sdf, (B,) + sdf.shape[1:]))
    for io in ('f32', 'f64'):
      ref = run(be, p, th, sdf, 0.0, th, io)
      assert ref[0][:, MO.COL['in_coll']].min() == 0 and ref[0][:, MO.COL['in_coll']].max() == 1
      for what, kw in (('again', dict(sdf=sdf)), ('tiled shared', dict(sdf=sdf, tiled=True)), ('per-sample', dict(sdf=per)), ('tiled per-sample', dict(sdf=per, tiled=True))):
        got = run(be, p, th, kw['sdf'], 0.0, th, io, tiled=kw.get('tiled', False))
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (dof, io, what)
    # per-sample grids that differ: every trajectory reads its own
    per2 = PC.rnd(per + rs.uniform(-0.3, 0.3, (B, 1, 1, 1)), 'f32')
    got, got_oe = run(be, p, th, per2, 0.0, None, 'f64')
    M, oe = MO.metrics(p, th, per2, 0.0, None)
    assert np.array_equal(got[:, EXACT], M[:, EXACT]) and np.array_equal(got_oe, oe)
    assert np.array_equal(run(be, p, th, per2, 0.0, None, 'f64', tiled=True)[1], got_oe)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_consistent_with_eval_errors(be, io):
  """sum(obs_error^2) / (2 n) is the unweighted obstacle error of dgp_eval_errors run with eps = metric_eps (plan_layer.py:379-382) and gp_mse d / 2 its unweighted GP
  error (:374-377): the bound of the existing unweighted-error test, TOL_ERR x 10 (parity_cases.py:1016)"""
  for dof, n in ((2, 64), (3, 33), (2, 300)):
    bt = LM.make(dof, 16 if n <= 64 else 64, 4 if n <= 64 else 5, n, 'static', vel=False, waves=64, nan=False, io='f32')
    eps = 0.25
    got, oe = run(be, bt.p, bt.th, bt.sdf, eps, None, io)
    ev = be.eval_errors(bt.p, bt.th, bt.start, bt.goal, bt.sdf, eps=np.full((bt.B, n, 1, 1), eps), io=io)
    unw_gp, unw_obs = ev[3], ev[4]
    e_obs = rel_err(np.sum(oe ** 2, axis=1) / (2.0 * n), unw_obs)
    e_gp = rel_err(got[:, MO.COL['gp_mse']] * (2 * dof) / 2.0, unw_gp)
    print('dof %d n %d %s: unw_obs %.3g unw_gp %.3g' % (dof, n, io, e_obs, e_gp))
    assert e_obs < PC.TOL_ERR[io] * 10 and e_gp < PC.TOL_ERR[io] * 10, (dof, n, io, e_obs, e_gp)


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_other_constants(be, golden, io):
  """dgp_traj_metrics at parity_cases.ND (x_lims (-3, 8), y_lims (-4, 6), total_time_sec 7, radius 0.3) with velocity limits v_x = 0.6 != v_y = 0.9, on the 33 x 37 grid
  stored row-major and tiled: against the reference's own rows (tests/golden/g11_config_constants.npz, fp64; fp32: tests/metrics_oracle.py on the rounded inputs) at
  the bounds of test_fixture_cases, and obs_error against the dgp_eval_errors path as test_consistent_with_eval_errors does."""
  g = golden('g11_config_constants')
  n = int(g['n'])
  p = PC.nd_params(2, n, **PC.ND_VEL)
  th, th_opt, sdf, eps = g['met_th'], g['met_th_opt'], g['sdf'], float(g['met_eps'])
  M, oe = g['met_metrics'], g['met_obs_error']
  M0, oe0 = MO.metrics(p, th, sdf, eps, th_opt)      # the inputs are fp32 numbers: one expectation for both I/O types
  tol = PC.TOL_ERR['f64']
  cv = MO.COL['constraint_violation']
  swapped = MO.metrics(PC.nd_params(2, n, use_vel_limits=True, v_x=p.v_y, v_y=p.v_x), th, sdf, eps)[0][:, cv]
  assert (swapped != M[:, cv]).sum() >= 2      # the column tells a handle with the two limits swapped from this one
  for tiled in (False, True):
    got, got_oe = run(be, p, th, sdf, eps, th_opt, io, tiled=tiled)
    for want, want_oe, ref in ((M, oe, 'reference'), (M0, oe0, 'oracle')):
      errs = {MO.NAMES[c]: rel_err(got[:, c], want[:, c]) for c in MO.REAL if np.max(np.abs(want[:, c])) > 0}
      print('other constants %s %s vs %s: worst %s; obs_error %.3g' % (io, 'tiled' if tiled else 'row-major', ref, max(errs.items(), key=lambda kv: kv[1]), rel_err(got_oe, want_oe)))
      np.testing.assert_array_equal(got[:, EXACT], want[:, EXACT])
      for c in MO.REAL:
        if np.max(np.abs(want[:, c])) == 0: assert not got[:, c].any(), (io, MO.NAMES[c])
        else: assert errs[MO.NAMES[c]] < tol, (io, tiled, ref, MO.NAMES[c], errs[MO.NAMES[c]])
      assert rel_err(got_oe, want_oe) < PC.TOL_ERR[io], (io, tiled, ref, 'obs_error')
      if io == 'f64': np.testing.assert_array_equal(got_oe, want_oe)
    B = th.shape[0]
    ev = be.eval_errors(p, th, th[:, :1], th[:, -1:], sdf, eps=np.full((B, n, 1, 1), eps), io=io)
    e_obs, e_gp = rel_err(np.sum(got_oe ** 2, axis=1) / (2.0 * n), ev[4]), rel_err(got[:, MO.COL['gp_mse']] * 4 / 2.0, ev[3])
    print('other constants %s: unw_obs %.3g unw_gp %.3g' % (io, e_obs, e_gp))
    assert e_obs < PC.TOL_ERR[io] * 10 and e_gp < PC.TOL_ERR[io] * 10, (io, e_obs, e_gp)


def _mini_planner_and_batch(env=0, dtype=torch.float64):
  """the problems of one environment of the mini dataset (the two environments' grids differ in size) as one batch, and a planner for it"""
  from dgpmp2_amd.datasets.planning_dataset import PlanningDataset
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  root = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mini_dataset')
  ds = PlanningDataset(root, 'train')
  samples = [ds[i] for i in range(len(ds))]
  shapes = sorted({tuple(s_['sdf'].shape) for s_ in samples})
  samples = [s_ for s_ in samples if tuple(s_['sdf'].shape) == shapes[env]]
  assert len(shapes) == 2 and len(samples) == 2
  dev = 'cuda:0'
  cat = lambda k: torch.stack([s[k] for s in samples]).to(dtype).to(dev)
  sdf, start, goal, th_opt = cat('sdf'), cat('start'), cat('goal'), cat('th_opt')
  B, n = th_opt.shape[:2]
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01), 'K_v': t(0.01), 'v_x': [1.0], 'v_y': [1.0]}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1, 'use_vel_limits': True}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': 5, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  planner = DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), B, n, use_cuda=True), batch_size=B, use_cuda=True)
  return planner, sdf, start, goal, th_opt


@pytest.mark.parametrize('env', [0, 1])
def test_planner_trajectory_metrics_after_forward_on_the_mini_dataset(env):
  from dgpmp2_amd.utils.planner_utils import straight_line_trajb
  planner, sdf, start, goal, th_opt = _mini_planner_and_batch(env)
  B, n = th_opt.shape[:2]
  th_init = straight_line_trajb(start[:, :, :2], goal[:, :, :2], 10.0, n - 1, 2)
  th_final = planner.forward(th_init, start, goal, (sdf > 0).to(sdf.dtype), sdf)[0]
  r = planner.trajectory_metrics(th_final, sdf, th_opt, return_obs_error=True)
  assert r.raw.shape == (B, 13) and r.raw.dtype == torch.float64 and r.raw.is_cuda and r.in_collision.dtype == torch.bool and r.num_penetrating.dtype == torch.int64
  p = O.OracleParams(dof=2, total_time_step=n - 1, use_vel_limits=True)
  M, oe = MO.metrics(p, th_final.cpu().numpy(), sdf.cpu().numpy(), 0.0, th_opt.cpu().numpy())
  got = r.raw.cpu().numpy()
  assert np.array_equal(got[:, EXACT], M[:, EXACT]) and np.array_equal(r.obs_error.cpu().numpy(), oe)
  for c in MO.REAL:
    assert np.max(np.abs(got[:, c] - M[:, c])) <= PC.TOL_ERR['f64'] * max(np.max(np.abs(M[:, c])), 1e-300), MO.NAMES[c]
  assert r.in_collision.tolist() == [bool(v) for v in M[:, MO.COL['in_coll']]] and r.num_penetrating.tolist() == [int(v) for v in M[:, MO.COL['num_penetrating']]]
  for k in ('coll_intensity', 'max_penetration', 'avg_penetration', 'gp_mse', 'avg_vel', 'avg_acc', 'avg_jerk', 'constraint_violation'):
    assert torch.equal(r[k], r.raw[:, MO.COL[k]])
  # one trajectory at a time with the host-side mirrors, the way the reference's loop scores it
  from dgpmp2_amd.utils.planner_utils import smoothness_metrics, collision_metrics
  for b in range(B):
    v, a, j = smoothness_metrics(th_final[b], 10.0, n - 1)
    ic, ap, mp, ci = collision_metrics(th_final[b], r.obs_error[b].reshape(n, 1, 1), 10.0, n - 1)
    for want, k in ((v, 'avg_vel'), (a, 'avg_acc'), (j, 'avg_jerk'), (ap, 'avg_penetration'), (mp, 'max_penetration'), (ci, 'coll_intensity')):
      assert abs(float(want) - float(r[k][b])) <= 1e-11 * max(abs(float(want)), 1e-300) or float(want) == float(r[k][b]), (b, k)
    assert ic == bool(r.in_collision[b])
  # float32 tensors, a tiled grid and an expand()ed shared grid go the same way as in step()
  from dgpmp2_amd.utils.sdf_utils import tile_sdf
  r32 = planner.trajectory_metrics(th_final.float(), sdf.float(), th_opt.float())
  r32t = planner.trajectory_metrics(th_final.float(), tile_sdf(sdf.float()), th_opt.float())
  assert torch.equal(r32.raw, r32t.raw)
  one = planner.trajectory_metrics(th_final, sdf[:1].expand(B, *sdf.shape[1:]), th_opt)
  assert torch.equal(one.raw[0], r.raw[0])


def test_trajectory_metrics_capture_and_replay():
  planner, sdf, start, goal, th_opt = _mini_planner_and_batch()
  B, n = th_opt.shape[:2]
  th = th_opt + 0.05 * torch.randn_like(th_opt)
  score = lambda t: planner.trajectory_metrics(t, sdf, th_opt, eps=0.1, return_obs_error=True)
  with torch.no_grad():
    eager = score(th)
    static_in = th.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      score(static_in)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out = score(static_in)
      coll, count = out.in_collision, out.num_penetrating
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.raw, eager.raw) and torch.equal(out.obs_error, eager.obs_error)
    assert torch.equal(coll, eager.in_collision) and torch.equal(count, eager.num_penetrating)
    th2 = th_opt.clone()
    static_in.copy_(th2)
    graph.replay()
    torch.cuda.synchronize()
    again = score(th2)
    assert torch.equal(out.raw, again.raw) and not out.raw[:, MO.COL['traj_mse']].any()
  # inside planner.graphed_iteration
  it = planner.graphed_iteration(lambda t: planner.trajectory_metrics(t, sdf, th_opt, eps=0.1).raw)
  with torch.no_grad():
    res = it(th).clone()
    res2 = it(th_opt)
  assert torch.equal(res, eager.raw) and torch.equal(res2, again.raw)
