"""CPU-only tests of the trajectory-metrics feature (dgp_traj_metrics and what sits on top of it): the Python mirrors of the reference's metric functions and
tests/metrics_oracle.py against the fixture tests/golden/g9_metrics.npz (the reference's own numbers, tests/golden/make_metrics_golden.py), host-side argument
validation of the entry point, the marshalling of PlanLayer.trajectory_metrics against a recording stand-in for the trampoline, and the CPU emulator library
still loading through the shared binding with the entry point reported as absent.  The kernel itself: tests/test_hip_metrics.py (-m gpu)."""
import numpy as np
import pytest
import torch

import harness
import metrics_oracle as MO
from metrics_oracle import load_case, case_names
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2 import plan_layer as PL
from dgpmp2_amd.robot_models import PointRobot2D
from dgpmp2_amd.utils import planner_utils as PU, sdf_utils as SU
from oracle import gpmp2_oracle as O


def test_fixture_holds_the_issue_cases(golden):
  g = golden('g9_metrics')
  assert tuple(str(s) for s in g['names']) == MO.NAMES == _capi.METRIC_NAMES
  shapes = {c: (int(g[c + '_dof']), int(g[c + '_n'])) for c in case_names(g)}
  assert sorted(v for c, v in shapes.items() if c != 'tie') == [(2, 4), (2, 33), (2, 64), (2, 101), (3, 64)]
  assert sorted({float(g[c + '_eps']) for c in case_names(g)}) == [0.0, 0.4]
  assert any(tuple(g[c + '_hw'])[0] != tuple(g[c + '_hw'])[1] for c in case_names(g))      # the non-square grid
  for c in case_names(g):
    B = g[c + '_th'].shape[0]
    assert (6 <= B <= 8 or c == 'tie') and g[c + '_metrics'].shape == (B, 13)
    np.testing.assert_array_equal(g[c + '_ref_num_penetrating'], 1.5 * g[c + '_metrics'][:, MO.COL['num_penetrating']])      # numel(nonzero of (n-2,1,1)) / 2


def test_python_mirrors_against_the_reference(golden):
  """smoothness_metrics / collision_metrics of dgpmp2_amd.utils.planner_utils, called as learning/test_planner.py:300-304 calls the reference's"""
  g = golden('g9_metrics')
  C = MO.COL
  for name in case_names(g):
    p, th, th_opt, sdf, eps, M, oe, ref_num = load_case(g, name)
    steps = p.n - 1
    for b in range(th.shape[0]):
      traj = torch.from_numpy(th[b])
      v, a, j = PU.smoothness_metrics(traj, p.total_time_sec, steps)
      for got, col in ((v, 'avg_vel'), (a, 'avg_acc'), (j, 'avg_jerk')):
        assert abs(got.item() - M[b, C[col]]) <= 1e-14 * max(1.0, abs(M[b, C[col]])), (name, b, col)
      err = torch.from_numpy(oe[b]).reshape(p.n, 1, 1)                 # obs_error[0] of ObstacleFactor.get_error
      in_coll, avg_pen, max_pen, ci = PU.collision_metrics(traj, err, p.total_time_sec, steps)
      assert isinstance(in_coll, bool) and in_coll == bool(M[b, C['in_coll']])
      assert avg_pen.item() == M[b, C['avg_penetration']] and max_pen.item() == M[b, C['max_penetration']] and ci == M[b, C['coll_intensity']], (name, b)
      # an (n,1) tensor gives the plain count: the factor 1.5 is the caller's (n,1,1) shape
      assert PU.collision_metrics(traj, err.reshape(p.n, 1), p.total_time_sec, steps)[3] * 1.5 == pytest.approx(ci, rel=1e-15, abs=0)


def test_path_to_traj_avg_vel_costmap_and_safe_sdf():
  path = [np.array([0.0, 1.0]), np.array([1.0, 1.5]), np.array([4.0, 3.0])]
  th = PU.path_to_traj_avg_vel(path, 2.0, 2)
  assert th.shape == (3, 4) and th.dtype == torch.get_default_dtype()
  assert torch.equal(th[:, :2], torch.tensor([[0.0, 1.0], [1.0, 1.5], [4.0, 3.0]])) and torch.equal(th[:, 2:], torch.tensor([[2.0, 1.0]] * 3))
  sdf = torch.tensor([[0.5, 0.2], [-0.1, 0.3]], dtype=torch.float64)
  assert torch.equal(SU.safe_sdf(sdf, 0.3), -1.0 * sdf + 0.3)
  assert torch.equal(SU.costmap_2d(sdf, 0.3), torch.tensor([[0.0, 0.3 - 0.2], [0.3 + 0.1, 0.0]], dtype=torch.float64))


def test_metrics_oracle_against_the_reference(golden):
  g = golden('g9_metrics')
  for name in case_names(g):
    p, th, th_opt, sdf, eps, M, oe, _ = load_case(g, name)
    for reverse in (False, True):
      got, got_oe = MO.metrics(p, th, sdf, eps, th_opt, reverse=reverse)
      np.testing.assert_array_equal(got[:, [MO.COL['in_coll'], MO.COL['num_penetrating']]], M[:, [MO.COL['in_coll'], MO.COL['num_penetrating']]])
      np.testing.assert_array_equal(got_oe, oe)                        # same operation order as the reference's lookup
      for c in MO.REAL:
        assert np.max(np.abs(got[:, c] - M[:, c])) <= 1e-13 * max(np.max(np.abs(M[:, c])), 1e-300), (name, MO.NAMES[c], reverse)
    z, _ = MO.metrics(p, th, sdf, eps, None)
    assert not z[:, [MO.COL['pos_mse'], MO.COL['vel_mse'], MO.COL['traj_mse']]].any()


def _cfg(**kw):
  base = dict(num_states=64, dof=2, io_dtype=_capi.DGP_F32, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4,
              Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4)
  base.update(kw)
  return _capi.make_config(**base)


def test_entry_point_validates_arguments_without_gpu():
  """every call below fails validation, so nothing is launched"""
  api = _capi.get_api()
  assert 'traj_metrics' in _capi.CApi.SYMBOLS and api.traj_metrics is not None and api.abi_version() == 7
  s = _capi.Solver(_cfg())
  ok = s.sdf_arg(0x1000, 256, 256, 0)

  def code(*a, **kw):
    with pytest.raises(_capi.DgpError) as e:
      s.traj_metrics(*a, **kw)
    assert len(str(e.value)) > 20
    return e.value.code
  assert code(8, None, ok, metrics=0x1000) == _capi.DGP_EINVAL                                             # th
  assert code(8, 0x1000, s.sdf_arg(None, 256, 256, 0), metrics=0x1000) == _capi.DGP_EINVAL                # sdf->data
  assert api.traj_metrics(s.handle, 8, 0x1000, None, 0.0, None, 0x1000, None, None) == _capi.DGP_EINVAL   # sdf
  assert code(8, 0x1000, s.sdf_arg(0x1000, 64, 1, 0), metrics=0x1000) == _capi.DGP_EUNSUPPORTED           # single-column grid
  assert code(0, 0x1000, ok, metrics=0x1000) == _capi.DGP_EINVAL and code(-3, 0x1000, ok, metrics=0x1000) == _capi.DGP_EINVAL
  assert code(8, 0x1000, ok) == _capi.DGP_EINVAL                                                          # no output at all
  assert code(8, 0x1000, s.sdf_arg(0x1000, 256, 256, 0, layout=7), metrics=0x1000) == _capi.DGP_EINVAL
  assert api.traj_metrics(None, 8, 0x1000, ok, 0.0, None, 0x1000, None, None) == _capi.DGP_EINVAL         # handle
  s2 = _capi.Solver(_cfg(num_states=2))
  with pytest.raises(_capi.DgpError) as e:                                                                 # n = 2 has no interior state
    s2.traj_metrics(8, 0x1000, ok, metrics=0x1000)
  assert e.value.code == _capi.DGP_EINVAL and 'interior' in str(e.value)
  # a request of dgp_time_next_launch does not survive a rejected call
  assert api.time_next_launch(0x10, 0x20) == _capi.DGP_OK
  assert code(0, 0x1000, ok, metrics=0x1000) == _capi.DGP_EINVAL
  # ... whichever translation unit rejects it: the solver's entry points, the problem sampler, the obstacle-map generator (null handle)
  for call in (lambda: api.gn_step(None, 8, 0x1000, 0x1000, 0x1000, ok, None, 0x1000, None, None, None, None),
               lambda: api.sample_problems(None, 8, ok, None, None, 1, 0, None, 0x1000, 0x1000, 0x1000, None, None, None),
               lambda: api.obstacle_maps(None, 2, 32, 32, None, 1, 1, 0, None, None, 0, 0x1000, _capi.DGP_U8, None, None, None, None, None)):
    assert api.time_next_launch(0x10, 0x20) == _capi.DGP_OK
    assert call() == _capi.DGP_EINVAL and b'null handle' in api.last_error()
  assert api.time_next_launch(None, None) == _capi.DGP_OK


def test_trampoline_argument_count_and_null_handle():
  pc = _capi.get_pycall()
  with pytest.raises(TypeError):
    pc.traj_metrics(*([0] * 14))
  assert pc.traj_metrics(0, 1, 0x1000, 0x1000, 8, 8, 0, 0, 0, None, 0.0, None, 0x1000, None, 0) == _capi.DGP_EINVAL
  assert b'null' in _capi.get_api().last_error()
  # the ctypes stand-in of the trampoline takes the same positional arguments
  assert _capi.CtypesPycall(_capi.get_api()).traj_metrics(0, 1, 0x1000, 0x1000, 8, 8, 0, 0, 0, None, 0.0, None, 0x1000, None, 0) == _capi.DGP_EINVAL


def test_emulator_library_loads_and_reports_the_entry_point_as_absent():
  api = harness.emul_api()                                             # _capi.CApi(libgn_emul.so, 'emul_'): every other symbol is bound
  assert api.prefix == 'emul_' and api.abi_version() == _capi.DGP_ABI_VERSION == 7
  assert api.traj_metrics is None and api.gn_step is not None and api.sdf_2d is not None
  s = _capi.Solver(_cfg(), api=api)
  with pytest.raises(NotImplementedError, match='emul_traj_metrics'):
    s.traj_metrics(8, 0x1000, s.sdf_arg(0x1000, 8, 8, 0), metrics=0x1000)


class RecordingPycall(object):
  def __init__(self): self.calls = []

  def traj_metrics(self, *a):
    assert len(a) == 15, len(a)                                        # as csrc/dgp_pycall.c unpacks them
    self.calls.append(a)
    return 0


@pytest.fixture
def layer(monkeypatch):
  monkeypatch.setattr(PL, '_require_cuda', lambda t, name: None)
  monkeypatch.setattr(PL, '_cur_dev', lambda: -1)
  monkeypatch.setattr(PL, '_raw_stream', lambda i: 77)
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  n = 16
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  pl = PL.PlanLayer(gp, ob, pp, op, {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}, PointRobot2D(t(0.4), 1, n))
  pl.__dict__['_pc'] = RecordingPycall()
  return pl


def test_trajectory_metrics_marshalling(layer):
  B, n = 3, 16
  th = torch.randn(B, n, 4, dtype=torch.float32, requires_grad=True)
  opt = torch.randn(B, n, 4, dtype=torch.float32)
  sdf = torch.randn(1, 1, 8, 10, dtype=torch.float32)
  r = layer.trajectory_metrics(th, sdf.expand(B, 1, 8, 10))
  a = layer._pc.calls[-1]
  h = layer._solvers[torch.float32].h
  assert a[0] == h and a[1] == B and a[2] == th.data_ptr()
  assert a[3:10] == (sdf.data_ptr(), 8, 10, 0, _capi.DGP_SDF_ROWMAJOR, 0, None)                            # shared grid: stride 0
  assert a[10] == 0.0 and isinstance(a[10], float) and a[11] is None                                      # the reference's metrics epsilon; no expert trajectory
  assert a[12] == r.raw.data_ptr() and a[13] is None and a[14] == 77
  assert r.raw.shape == (B, _capi.DGP_METRIC_COUNT) == (B, 13) and r.raw.dtype == torch.float64 and not r.raw.requires_grad and r.obs_error is None
  # the named results: (B,) tensors, views of raw except the two typed ones
  r.raw.copy_(torch.arange(B * 13, dtype=torch.float64).reshape(B, 13))
  r.raw[:, 4] = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64)
  for i, name in enumerate(_capi.METRIC_NAMES):
    if name == 'in_coll': continue
    assert torch.equal(r[name].to(torch.float64), r.raw[:, i]) and getattr(r, name).shape == (B,)
  assert r.in_collision.dtype == torch.bool and r.in_collision.tolist() == [False, True, True]
  assert r.num_penetrating.dtype == torch.int64 and r.num_penetrating.tolist() == [5, 18, 31]
  assert r.gp_mse.data_ptr() == r.raw[:, 3].data_ptr()
  assert set(r.as_dict()) >= {'in_collision', 'coll_intensity', 'max_penetration', 'avg_penetration', 'gp_mse', 'avg_vel', 'avg_acc', 'avg_jerk', 'constraint_violation'}
  with pytest.raises(AttributeError):
    r.no_such_metric
  # per-sample grids, expert trajectories, a metrics epsilon, the raw obstacle errors
  per = torch.randn(B, 1, 8, 10, dtype=torch.float32)
  r = layer.trajectory_metrics(th, per, opt, eps=0.4, return_obs_error=True)
  a = layer._pc.calls[-1]
  assert a[3:7] == (per.data_ptr(), 8, 10, 80) and a[10] == 0.4 and a[11] == opt.data_ptr() and a[13] == r.obs_error.data_ptr()
  assert r.obs_error.shape == (B, n) and r.obs_error.dtype == torch.float32
  # float64 trajectories get the float64 handle; a tiled grid goes down as tiles
  from dgpmp2_amd.utils.sdf_utils import tile_sdf
  t = tile_sdf(torch.randn(B, 1, 10, 13, dtype=torch.float64))
  r = layer.trajectory_metrics(th.detach().double(), t)
  a = layer._pc.calls[-1]
  assert a[0] == layer._solvers[torch.float64].h and a[3:8] == (t.data_ptr(), 10, 13, 3 * 4 * 16, _capi.DGP_SDF_TILED4)
  # a non-contiguous trajectory tensor is made contiguous, not read with the wrong strides
  wide = torch.randn(B, n, 8, dtype=torch.float32)
  layer.trajectory_metrics(wide[:, :, :4], per)
  assert layer._pc.calls[-1][2] != wide.data_ptr()
  with pytest.raises(ValueError):
    layer.trajectory_metrics(th[:, :5], per)
  with pytest.raises(ValueError):
    layer.trajectory_metrics(th, per, opt[:2])
  with pytest.raises(TypeError):
    layer.trajectory_metrics(th, per, opt.double())
  with pytest.raises(ValueError):
    layer.trajectory_metrics(th, None)
  with pytest.raises(ValueError):
    layer.trajectory_metrics(th, torch.randn(2, 1, 8, 10))             # fewer grids than trajectories
