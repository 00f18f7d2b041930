"""CPU-only tests away from the default configuration constants (parity_cases.ND: another horizon, K_s != K_g, unsymmetric and unequal x and y limits, another
sigma, epsilon, radius and damping; velocity limits v_x != v_y; the non-holonomic weight).

  * the oracles -- oracle.gpmp2_oracle, oracle/gn_blocktri.c (fp64 and extended), oracle.autograd_torch, tests/metrics_oracle.py, tests/problems_oracle.py -- against
    the reference's own numbers at those constants (tests/golden/g11_config_constants.npz, made by tests/golden/make_config_golden.py), at the bounds the fixture
    tests of the same functions use at the default constants;
  * the sensitivity guard: on the inputs the GPU parity case uses (parity_cases.nondefault_inputs), putting any ONE constant back to its default moves the C oracle's
    dtheta by at least 1e-3 relative (100 x the fp32 parity bound) and err_ext by at least 1e-4 in every configuration that reads the constant -- so a kernel or
    host table that read the default, the other limit or the other weight could not pass the parity case; y_lims[1], which no GN kernel reads, is held by the
    sampler's guard: each of the four limits and an x / y swap changes at least half of the problems of the sampler's inputs (problems_cases.mixed_nd);
  * the marshalling of PlanLayer's configuration, field by field with every value distinct, and of generate_dataset's cell size and meta limits."""
import numpy as np
import pytest
import torch

import metrics_oracle as MO
import parity_cases as PC
import problems_cases as PCS
import problems_oracle as PO
from conftest import rel_err
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2 import plan_layer as PL
from oracle import gpmp2_oracle as O, blocktri as BT

TOL = 1e-9      # tests/test_oracle_golden.py


@pytest.fixture(scope='module')
def g(golden):
  return golden('g11_config_constants')


def _p(g, key, n):
  if key == 'xyh': return PC.nd_params(3, n, Q_c_inv=g['xyh_Q_c_inv'])
  return PC.nd_params(2, n, Q_c_inv=g['Q_c_inv'], **(PC.ND_VEL if key == 'vel' else {}))


def test_fixture_inputs_are_the_shared_builders(g):
  n = int(g['n'])
  x = PC.nondefault_inputs(2, n, 4, 'perstate', 'f32')
  for k, v in (('th', x.th), ('start', x.start), ('goal', x.goal), ('sdf', x.sdf), ('qc', x.qc), ('ow', x.ow.reshape(4, n, 1, 1)), ('eps', x.eps.reshape(4, n, 1, 1))):
    assert np.array_equal(g[k], v), k
  x3 = PC.nondefault_inputs(3, n, 4, 'static', 'f32')
  assert np.array_equal(g['xyh_th'], x3.th) and np.array_equal(g['xyh_start'], x3.start) and np.array_equal(g['xyh_goal'], x3.goal)
  assert g['sdf'].shape == (1, 1) + PC.ND_HW and g['sdf'].nbytes < 16384 and np.array_equal(g['met_th'][:4], x.th)
  # nothing is at its default; the pairs the defaults cannot tell apart differ
  assert all(PC.ND[k] != PC.ND_DEFAULT[k] for k in PC.ND if k in PC.ND_DEFAULT) and all(PC.ND_VEL[k] != PC.ND_DEFAULT[k] for k in ('K_v', 'v_x', 'v_y')) and PC.ND_DYN['K_d'] != PC.ND_DEFAULT['K_d']
  (x0, x1), (y0, y1) = PC.ND['x_lims'], PC.ND['y_lims']
  assert PC.ND['K_s'] != PC.ND['K_g'] and len({x0, x1, y0, y1, -x0, -y0, x1 - x0, y1 - y0}) == 8 and PC.ND_VEL['v_x'] != PC.ND_VEL['v_y']
  # the inputs reach the clamped band above row 0 and leave the grid (nondefault_inputs asserts it) and the grid is laid out by the pixel formula
  res = (x1 - x0) / PC.ND_HW[1]
  cx, cy, r = PC.ND_CIRCLES[0]
  px, py = -x0 / res + cx / res, -y0 / res - cy / res
  assert abs(PC.nd_grid()[0, 0, int(round(py)), int(round(px))] + r) < res


def test_numpy_oracle_against_the_reference(g):
  n = int(g['n'])
  for key in ('static', 'cov', 'vel', 'xyh'):
    pre = 'xyh_' if key == 'xyh' else ''
    p = _p(g, key, n)
    B = g[pre + 'th'].shape[0]
    sq, so, se = p.static_covs(B)
    covs = (g['qc'], g['ow'], g['eps']) if key == 'cov' else (sq, so, se)
    sdf = np.broadcast_to(g['sdf'], (B,) + g['sdf'].shape[1:])
    dth, err, eex = O.plan_layer_forward(g[pre + 'th'], g[pre + 'start'], g[pre + 'goal'], sdf, *covs, p)
    assert rel_err(dth, g[key + '_dth']) < TOL and rel_err(err, g[key + '_err']) < 1e-12, key
    if key + '_errext' in g: assert rel_err(eex, g[key + '_errext']) < 1e-12, key
    if key in ('vel', 'xyh'): assert p.M == int(g[key + '_M'])
  p = _p(g, 'static', n)
  usg, ugp, uob = O.unweighted_errors_batch(g['th'], g['start'], g['goal'], np.broadcast_to(g['sdf'], (4,) + g['sdf'].shape[1:]), p.static_covs(4)[2], p)
  assert usg.shape == g['unw_sg'].shape and ugp.shape == g['unw_gp'].shape and uob.shape == g['unw_obs'].shape
  assert rel_err(usg, g['unw_sg']) < 1e-12 and rel_err(ugp, g['unw_gp']) < 1e-12 and rel_err(uob, g['unw_obs']) < 1e-12


@pytest.mark.parametrize('extended', [False, True], ids=['fp64', 'extended'])
def test_blocktri_c_oracle_against_the_reference(g, extended):
  n = int(g['n'])
  for key in ('static', 'cov', 'vel', 'xyh'):
    pre = 'xyh_' if key == 'xyh' else ''
    B = g[pre + 'th'].shape[0]
    kw = dict(qc=g['qc'], ow=g['ow'].reshape(B, n), eps=g['eps'].reshape(B, n)) if key == 'cov' else {}
    dth, err, eex, info = BT.gn_step(_p(g, key, n), g[pre + 'th'], g[pre + 'start'], g[pre + 'goal'], g['sdf'], extended=extended, **kw)
    e = rel_err(dth, g[key + '_dth'])
    print('blocktri %s %s: dtheta %.3g err %.3g' % ('extended' if extended else 'fp64', key, e, rel_err(err, g[key + '_err'].reshape(-1))))
    assert not info.any() and e < TOL and rel_err(err, g[key + '_err'].reshape(-1)) < 1e-12, (key, e)
    if key + '_errext' in g: assert rel_err(eex, g[key + '_errext'].reshape(-1)) < 1e-12, key


def test_autograd_oracle_against_the_reference(g):
  from oracle import autograd_torch as AT
  n, B = int(g['n']), 4
  p = _p(g, 'cov', n)
  sdf = np.repeat(g['sdf'], B, 0)
  r = AT.step_gradients(p, g['th'], g['start'], g['goal'], sdf, g['gbar'], np.zeros(B), qc=g['qc'], ow=g['ow'], eps=g['eps'])
  assert rel_err(r['dtheta'], g['cov_dth']) < 1e-11
  for k in ('th', 'sdf', 'start', 'goal', 'qc', 'ow', 'eps'):
    assert rel_err(r[k].reshape(g['g_' + k].shape), g['g_' + k]) < 1e-10, (k, rel_err(r[k].reshape(g['g_' + k].shape), g['g_' + k]))
  r = AT.step_gradients(p, g['th'], g['start'], g['goal'], sdf, np.zeros_like(g['gbar']), g['gext'].reshape(B), qc=g['qc'], ow=g['ow'], eps=g['eps'])
  for k in ('th', 'sdf', 'start', 'goal', 'eps'):
    assert rel_err(r[k].reshape(g['ge_' + k].shape), g['ge_' + k]) < 1e-12, k
  assert np.all(r['qc'] == 0) and np.all(r['ow'] == 0) and bool(g['ge_none_qc']) and bool(g['ge_none_ow']) and not bool(g['err_requires_grad'])


def test_metrics_oracle_against_the_reference(g):
  n = int(g['n'])
  p = PC.nd_params(2, n, **PC.ND_VEL)
  M, oe = g['met_metrics'], g['met_obs_error']
  assert tuple(str(s) for s in g['met_names']) == MO.NAMES
  ex = [MO.COL['in_coll'], MO.COL['num_penetrating']]
  for reverse in (False, True):
    got, got_oe = MO.metrics(p, g['met_th'], g['sdf'], float(g['met_eps']), g['met_th_opt'], reverse=reverse)
    np.testing.assert_array_equal(got[:, ex], M[:, ex])
    np.testing.assert_array_equal(got_oe, oe)
    for c in MO.REAL:
      assert np.max(np.abs(got[:, c] - M[:, c])) <= 1e-13 * max(np.max(np.abs(M[:, c])), 1e-300), (MO.NAMES[c], reverse)
  # the two velocity limits are told apart: with them swapped the violation column differs
  sw, _ = MO.metrics(PC.nd_params(2, n, use_vel_limits=True, v_x=PC.ND_VEL['v_y'], v_y=PC.ND_VEL['v_x']), g['met_th'], g['sdf'], float(g['met_eps']))
  c = MO.COL['constraint_violation']
  assert (sw[:, c] != M[:, c]).sum() >= 2 and M[:, MO.COL['in_coll']].min() == 0 and M[:, MO.COL['in_coll']].max() == 1


def test_problems_oracle_against_the_reference(g):
  total = 0
  for f in g['env_fields']:
    sdf, pts, dist, want = g['env_%s_sdf' % f], g['env_%s_points' % f], g['env_%s_dist' % f], g['env_%s_feasible' % f]
    assert sdf.shape == PCS.ND_HW
    got_d = np.array([PO.signed_distance(sdf, q[0], q[1], PCS.ND_X, PCS.ND_Y) for q in pts])
    got = np.array([PO.is_feasible(sdf, q[0], q[1], float(g['env_clearance']), PCS.ND_X, PCS.ND_Y) for q in pts])
    assert np.array_equal(got_d, dist), f      # bit for bit, as tests/test_problems_oracle.py holds it at the default limits
    assert np.array_equal(got, want), f
    outside = ~((pts[:, 0] >= PCS.ND_X[0]) & (pts[:, 0] <= PCS.ND_X[1]) & (pts[:, 1] >= PCS.ND_Y[0]) & (pts[:, 1] <= PCS.ND_Y[1]))
    assert outside.sum() >= 12 and (got_d[outside] == PCS.ND_X[1] - PCS.ND_X[0]).all() and want[~outside].any() and not want[~outside].all()
    total += len(pts)
  assert total >= 300
  for n in (3, 16):
    got = PO.th_init_of(g['line_start'], g['line_goal'], n, float(g['line_total_time_sec']))
    assert got.dtype == np.float64 and np.array_equal(got, g['line_th_n%d' % n]), n
  assert float(g['line_total_time_sec']) == PCS.ND_T_SEC == 7.0


# ---- the sensitivity guards --------------------------------------------------------------------------------------------------------------------------------------

BASE = ('total_time_sec', 'K_s', 'K_g', 'cost_sigma', 'epsilon_dist', 'radius', 'reg', 'x_lims[0]', 'x_lims[1]', 'y_lims[0]')
# (name, dof, covariances, extra parameters, the constants the configuration's dtheta reads, those its err_ext reads)
GUARD = [('static + velocity limits', 2, 'static', PC.ND_VEL, BASE + ('K_v', 'v_x', 'v_y'), BASE + ('K_v', 'v_x', 'v_y')),
         ('xyh, non-holonomic', 3, 'static', {}, BASE + ('K_d',), BASE + ('K_d',)),
         # per-state tensors replace the static weight and epsilon in the step; err_ext keeps the fixed weight (plan_layer.py:310-345) and takes the tensors' epsilons
         ('per-state tensors', 2, 'perstate', {}, tuple(k for k in BASE if k not in ('cost_sigma', 'epsilon_dist')), tuple(k for k in BASE if k != 'epsilon_dist'))]


def _back_to_default(kw, name):
  kw = dict(kw)
  if '[' in name:
    k, i = name[:6], int(name[7])
    lims = list(kw[k]); lims[i] = (-5.0, 5.0)[i]; kw[k] = tuple(lims)
  else:
    kw[name] = PC.ND_DEFAULT[name]
  return kw


@pytest.mark.parametrize('n', [13, 61])
def test_every_constant_moves_the_oracle(n):
  """Smallest relative move of (dtheta, err_ext) over the three configurations and both lengths when ONE constant goes back to its default:
  total_time_sec (0.30, 2.8e-4), K_s (1.5e-3, 9.3e-2), K_g (2.5e-2, 0.44), cost_sigma (3.0e-2, 0.34), epsilon_dist (0.11, 1.6e-2), radius (0.10, 1.0e-2), reg (1.4e-2, -),
  x_lims[0] (0.52, 2.9e-2), x_lims[1] (0.75, 6.3e-3), y_lims[0] (1.06, 3.6e-2), K_v (6.3e-2, 0.39), v_x (0.64, 0.11), v_y (0.73, 1.9e-2), K_d (0.19, 2.0); y_lims[1] moves
  nothing here and every one of the sampler's 131 problems below."""
  B = 5
  for name, dof, cov, extra, reads_dth, reads_ext in GUARD:
    x = PC.nondefault_inputs(dof, n, B, cov, 'f32')
    sh = (B, n, 1, 1)
    okw = dict(qc=x.qc, ow=None if x.ow is None else x.ow.reshape(sh), eps=None if x.eps is None else x.eps.reshape(sh))
    base = dict(PC.ND, **(PC.ND_DYN if dof == 3 else {})); base.update(extra)
    run = lambda kw: BT.gn_step(O.OracleParams(dof=dof, total_time_step=n - 1, **kw), x.th, x.start, x.goal, x.sdf, **okw)
    r0 = run(base)
    assert not r0[3].any()
    for c in reads_dth:
      r = run(_back_to_default(base, c))
      m_d, m_x = rel_err(r[0], r0[0]), rel_err(r[2], r0[2])
      print('sensitivity n %d %-26s %-15s dtheta %.2e err_ext %.2e' % (n, name, c, m_d, m_x))
      assert m_d >= 1e-3, (name, n, c, m_d)
      if c != 'reg' and c in reads_ext: assert m_x >= 1e-4, (name, n, c, m_x)
    for c in set(reads_ext) - set(reads_dth):
      m_x = rel_err(run(_back_to_default(base, c))[2], r0[2])
      print('sensitivity n %d %-26s %-15s err_ext %.2e' % (n, name, c, m_x))
      assert m_x >= 1e-4, (name, n, c, m_x)
    # y_lims[1] is read by no GN kernel and no oracle of them: pinned by the sampler below
    r = run(_back_to_default(base, 'y_lims[1]'))
    assert np.array_equal(r[0], r0[0]) and np.array_equal(r[2], r0[2])


def test_every_limit_moves_the_sampled_problems():
  f, env, diag, (start, goal, draws, info) = PCS.mixed_nd()
  PCS.check_branches(PCS.branch_counts(env, diag, draws, info))      # the inputs of the GPU test take every branch at these limits too
  B = len(env)
  (x0, x1), (y0, y1) = PCS.ND_X, PCS.ND_Y
  for name, xl, yl in (('x_lims[0]', (-5.0, x1), PCS.ND_Y), ('x_lims[1]', (x0, 5.0), PCS.ND_Y), ('y_lims[0]', PCS.ND_X, (-5.0, y1)), ('y_lims[1]', PCS.ND_X, (y0, 5.0)),
                       ('x / y swapped', PCS.ND_Y, PCS.ND_X)):
    o = PCS.mixed_nd(x_lims=xl, y_lims=yl)[3]
    moved = int(((o[0] != start).any((1, 2)) | (o[1] != goal).any((1, 2))).sum())
    print('sampler sensitivity %-14s %d of %d problems differ' % (name, moved, B))
    assert 2 * moved >= B, (name, moved)
  _, _, sdiag, (_, _, _, sinfo) = PCS.shared_nd()
  assert ((sinfo & 8) != 0).sum() > 0 and (sdiag < 0).sum() > 0


# ---- marshalling -------------------------------------------------------------------------------------------------------------------------------------------------

def _layer(monkeypatch, dof, n=13):
  from dgpmp2_amd.robot_models import PointRobot2D, PointRobotXYH
  monkeypatch.setattr(PL, '_require_cuda', lambda t, name: None)
  monkeypatch.setattr(PL, '_cur_dev', lambda: -1)
  monkeypatch.setattr(PL, '_raw_stream', lambda i: 77)
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  qc = [[1.3, 0.4], [0.4, 0.9]] if dof == 2 else [[1.2, 0.2, -0.1], [0.2, 0.8, 0.35], [-0.1, 0.35, 2.0]]
  gp = {'Q_c_inv': t(qc), 'K_s': t(PC.ND['K_s']), 'K_g': t(PC.ND['K_g']), 'K_v': t(0.04), 'v_x': [0.6], 'v_y': [0.9], 'K_d': t(0.06)}      # (K_v, K_d: ND_VEL / ND_DYN repeat K_s / reg)
  ob = {'cost_sigma': t(PC.ND['cost_sigma']), 'epsilon_dist': t(PC.ND['epsilon_dist'])}
  pp = {'dof': dof, 'state_dim': 2 * dof, 'total_time_sec': PC.ND['total_time_sec'], 'total_time_step': n - 1, 'use_vel_limits': dof == 2, 'non_holonomic': dof == 3}
  op = {'method': 'gauss_newton', 'reg': PC.ND['reg'], 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': list(PC.ND['x_lims']), 'y_lims': list(PC.ND['y_lims'])}
  robot = PointRobot2D(t(PC.ND['radius']), 1, n) if dof == 2 else PointRobotXYH(t(PC.ND['radius']), False, 1, n)
  return PL.PlanLayer(gp, ob, pp, op, env, robot), qc


@pytest.mark.parametrize('dof', [2, 3])
def test_plan_layer_configuration_field_by_field(monkeypatch, dof):
  n = 13
  layer, qc = _layer(monkeypatch, dof, n)
  for dtype, code in ((torch.float64, _capi.DGP_F64), (torch.float32, _capi.DGP_F32)):
    layer._solver(dtype)
    c = layer._solvers[dtype].cfg
    want = dict(total_time_sec=7.0, K_s=0.02, K_g=0.005, reg=0.05, sphere_radius=0.3, cost_sigma=0.03, epsilon_dist=0.25,
                K_v=0.04 if dof == 2 else 0.0, v_x=0.6 if dof == 2 else 0.0, v_y=0.9 if dof == 2 else 0.0, K_d=0.06 if dof == 3 else 0.0)
    vals = [v for v in want.values() if v != 0.0] + [-3.0, 8.0, -4.0, 6.0]
    assert len(set(vals)) == len(vals)      # every value distinct: a swapped pair of fields cannot pass
    for k, v in want.items(): assert getattr(c, k) == v, (k, getattr(c, k), v)
    assert (c.x_lims[0], c.x_lims[1], c.y_lims[0], c.y_lims[1]) == (-3.0, 8.0, -4.0, 6.0)
    assert [c.Q_c_inv[i] for i in range(9)] == [v for row in qc for v in row] + [0.0] * (9 - dof * dof)
    assert (c.num_states, c.dof, c.nlinks, c.io_dtype) == (n, dof, 1, code) and c.struct_size == __import__('ctypes').sizeof(_capi.DgpConfig)
    assert c.flags == (_capi.DGP_FLAG_VEL_LIMITS if dof == 2 else _capi.DGP_FLAG_NONHOLONOMIC)
  # tests/harness.py's configuration of the same constants: what every parity case above the C-ABI runs with
  import harness
  p = PC.nd_params(dof, n, Q_c_inv=np.array(qc), **(dict(PC.ND_VEL, K_v=0.04) if dof == 2 else dict(K_d=0.06)))
  h, c = harness.config_from_oracle(p, 'f64'), layer._solvers[torch.float64].cfg
  skip = ('K_d',) if dof == 2 else ('K_v', 'v_x', 'v_y')      # (the weight and limits of a factor that is switched off: PlanLayer sends zeros, the harness the oracle's defaults)
  for name, _ in _capi.DgpConfig._fields_:
    if name in skip: continue
    a, b = getattr(h, name), getattr(c, name)
    assert (list(a) == list(b)) if hasattr(a, '__len__') else (a == b), name


class _DeviceTensor(torch.Tensor):
  """a host tensor that says it lives on the device: generate_dataset's own check is all that reads it here"""
  is_cuda = property(lambda self: True)


def test_generate_dataset_cell_size_and_meta_limits_come_from_the_planner(monkeypatch, tmp_path):
  from dgpmp2_amd.datasets import problem_generation as PG, PlanningDataset
  from dgpmp2_amd.utils import sdf_utils as SU
  E, H, W, n, P = 2, 9, 22, 5, 2
  seen = {}

  def sdf_2d_batch(im, padlen=0, res=None):
    seen['res'], seen['padlen'] = res, padlen
    return torch.ones(E, H, W, dtype=torch.float64)

  def sample_problems(layer, sdf, B, env_index=None, seed=0, diagonal=None, **params):
    seen['layer'] = layer
    z = torch.zeros(B, 1, 4, dtype=torch.float64)
    return z, z + 1.0, torch.zeros(B, n, 4, dtype=torch.float64), PG.SampleInfo(torch.zeros(B, dtype=torch.int32), torch.zeros(B, 2, dtype=torch.int32))

  class Planner(object):
    env_params = {'x_lims': [-3.0, 8.0], 'y_lims': [-4.0, 6.0]}
    plan_layer = object()
    def forward(self, th, *a): return (th,)
    def trajectory_metrics(self, th, sdfb, eps=0.0): return type('M', (), {'in_collision': torch.zeros(th.shape[0], dtype=torch.bool)})()
  monkeypatch.setattr(SU, 'sdf_2d_batch', sdf_2d_batch)
  monkeypatch.setattr(PG, 'sample_problems', sample_problems)
  images = torch.ones(E, H, W, dtype=torch.float64).as_subclass(_DeviceTensor)
  r = PG.generate_dataset(str(tmp_path), 'train', images, Planner(), P)
  assert r['num_envs'] == E and seen['layer'] is Planner.plan_layer and seen['padlen'] == 0
  assert seen['res'] == (8.0 - (-3.0)) / W                      # the x span over the image WIDTH: not 10 / W, not the y span, not the height
  ds = PlanningDataset(str(tmp_path), 'train')
  assert ds.meta_data['env_params'] == {'x_lims': [-3.0, 8.0], 'y_lims': [-4.0, 6.0]} and ds.meta_data['im_size'] == W
