"""CPU-only tests of the GP interpolation feature (dgp_gp_interpolate and what sits on top of it): the closed form of include/dgpmp2_hip.h (tests/interp_oracle.py)
against its matrix definition for two SPD Q_c, straight lines, the copy rule, the torch mirror utils.planner_utils.gp_interpolate_traj, the motivating case pinned on
the oracle, host-side argument validation of the entry point, and the marshalling of PlanLayer.interpolate against a recording stand-in for the trampoline.
The kernel itself: tests/test_hip_interp.py (-m gpu).

The formula bound used throughout: 1e-12 x (largest |entry| of the two support states) x max(1, dt, 1 / dt) -- about ten fp64 operations per value with coefficients
of at most 6 / dt."""
import numpy as np
import pytest
import torch

import harness
import interp_cases as IC
import interp_oracle as IO_
import metrics_oracle as MO
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2 import plan_layer as PL
from dgpmp2_amd.robot_models import PointRobot2D
from dgpmp2_amd.utils import planner_utils as PU
from oracle import gpmp2_oracle as O

DTS, KS = (0.05, 10.0 / 63.0, 1.0), (1, 4, 7)


def bound(th, K, dt):
  """(B, N_d, 1): the formula bound of every dense state"""
  n = th.shape[1]
  i = np.arange(IO_.num_dense(n, K)) // (K + 1)
  big = np.abs(th).max(-1)
  return (1e-12 * np.maximum(big[:, i], big[:, np.minimum(i + 1, n - 1)]) * max(1.0, dt, 1.0 / dt))[:, :, None]


def random_spd(rs, dof):
  A = rs.randn(dof, dof)
  return A @ A.T + 0.5 * np.eye(dof)


@pytest.mark.parametrize('dof', [2, 3])
def test_closed_form_equals_the_matrix_definition_and_qc_cancels(dof):
  rs = np.random.RandomState(dof)
  n, B = 5, 4
  th = rs.randn(B, n, 2 * dof) * 3.0
  q1, q2 = random_spd(rs, dof), random_spd(rs, dof) * 7.0
  p = O.OracleParams(dof=dof, total_time_step=n - 1)
  for dt in DTS:
    for K in KS:
      got = IO_.dense(p, th, K, dt=dt)
      d1, d2 = IO_.dense_from_definition(p, th, K, q1, dt=dt), IO_.dense_from_definition(p, th, K, q2, dt=dt)
      bd = bound(th, K, dt)
      e1, e2, e12 = (np.abs(got - d1) / bd).max(), (np.abs(got - d2) / bd).max(), (np.abs(np.asarray(d1 - d2, np.float64)) / bd).max()
      print('dof %d dt %.4g K %d: closed form vs definition %.3g, %.3g of the bound; Q_c against Q_c %.3g' % (dof, dt, K, e1, e2, e12))
      assert e1 <= 1.0 and e2 <= 1.0 and e12 <= 1.0, (dof, dt, K, e1, e2, e12)
      assert got.shape == (B, (n - 1) * (K + 1) + 1, 2 * dof)


@pytest.mark.parametrize('dof', [2, 3])
def test_constant_velocity_line_interpolates_onto_itself(dof):
  rs = np.random.RandomState(10 + dof)
  B, n, T = 5, 9, 10.0
  start, goal = rs.uniform(-4, 4, (B, 1, dof)), rs.uniform(-4, 4, (B, 1, dof))
  th = O.straight_line_trajb(start, goal, T, n - 1, dof)
  p = O.OracleParams(dof=dof, total_time_sec=T, total_time_step=n - 1)
  for K in KS:
    want = O.straight_line_trajb(start, goal, T, (n - 1) * (K + 1), dof)      # the same line at the dense times
    got = IO_.dense(p, th, K)
    assert (np.abs(got - want) <= bound(th, K, p.dt)).all(), K
    np.testing.assert_allclose(IO_.times(p, K), np.arange(got.shape[1]) * T / (got.shape[1] - 1), rtol=0, atol=1e-13)


def planted(rs, B, n, d):
  th = rs.randn(B, n, d)
  th[0, 1, 0], th[1, n - 1, d - 1], th[2, 0, 1], th[2, 2, 2] = np.nan, np.nan, -0.0, -0.0
  return th


def test_k0_returns_th_itself_and_support_rows_are_bit_copies():
  rs = np.random.RandomState(3)
  for dof in (2, 3):
    B, n, d = 3, 4, 2 * dof
    th = planted(rs, B, n, d)
    p = O.OracleParams(dof=dof, total_time_step=n - 1)
    d0 = IO_.dense(p, th, 0)
    assert np.array_equal(d0, th, equal_nan=True) and np.array_equal(IC.bits(d0), IC.bits(th))
    t0 = PU.gp_interpolate_traj(torch.from_numpy(th), p.total_time_sec, n - 1, 0).numpy()
    assert np.array_equal(IC.bits(t0), IC.bits(th))
    for K in (1, 2, 4, 7):
      dk = IO_.dense(p, th, K)
      assert np.array_equal(IC.bits(dk[:, ::K + 1]), IC.bits(th)), K
      assert np.signbit(dk[2, 0, 1]) and np.signbit(dk[2, 2 * (K + 1), 2])      # -0.0 stays -0.0: the formula at s = 0 would give +0.0
      tk = PU.gp_interpolate_traj(torch.from_numpy(th), p.total_time_sec, n - 1, K).numpy()
      assert np.array_equal(IC.bits(tk[:, ::K + 1]), IC.bits(th)), K


@pytest.mark.parametrize('dof', [2, 3])
def test_torch_mirror_equals_the_oracle(dof):
  rs = np.random.RandomState(20 + dof)
  B, n = 6, 7
  th = rs.randn(B, n, 2 * dof) * 2.0
  for T in (0.05 * (n - 1), 10.0, 1.0 * (n - 1)):
    p = O.OracleParams(dof=dof, total_time_sec=T, total_time_step=n - 1)
    for K in (0,) + KS:
      want = IO_.dense(p, th, K)
      got = PU.gp_interpolate_traj(torch.from_numpy(th), T, n - 1, K)
      assert got.shape == want.shape and got.dtype == torch.float64
      assert (np.abs(got.numpy() - want) <= bound(th, K, p.dt)).all(), (T, K)
      np.testing.assert_allclose(PU.gp_interpolate_times(T, n - 1, K).numpy(), IO_.times(p, K), rtol=0, atol=1e-12 * T)
    g32 = PU.gp_interpolate_traj(torch.from_numpy(th).float(), T, n - 1, 4)
    assert g32.dtype == torch.float32 and np.abs(g32.numpy() - IO_.dense(p, th, 4)).max() < 1e-4 * max(1.0, 1.0 / p.dt)
  with pytest.raises(ValueError):
    PU.gp_interpolate_traj(torch.from_numpy(th), 10.0, n, 1)


def test_summary_definitions():
  c = np.array([[9.0, 0.0, 0.5, 2.0, 2.0, 0.0, 9.0],
                [9.0, 0.0, 0.0, 0.0, 0.0, 0.0, 9.0],
                [0.0, 1.0, np.nan, 3.0, np.nan, 0.0, 0.0]])
  S = IO_.summary(c)
  assert S[0].tolist() == [1.0, 3.0, 4.5 / 5.0, 2.0, 2.0, 3.0]            # the first and the last state are left out; the smallest index of the two maxima
  assert S[1].tolist() == [0.0, 0.0, 0.0, 0.0, -1.0, 1.0]
  assert S[2, :2].tolist() == [1.0, 4.0] and np.isnan(S[2, 2]) and np.isnan(S[2, 3]) and S[2, 4:].tolist() == [1.0, 2.0]      # a NaN counts, and wins
  assert IO_.NAMES == _capi.DENSE_NAMES and _capi.DGP_DENSE_COUNT == 6 and [_capi.DGP_DENSE_IN_COLL, _capi.DGP_DENSE_WORST_INDEX] == [0, 5]
  assert {IO_.lpt(nd) for nd in (2, 64, 65, 128, 129, 1033)} == {16, 32, 64} and IO_.lpt(64) == 16 and IO_.lpt(65) == 32 and IO_.lpt(129) == 64


def test_motivating_case_on_the_oracle():
  """the support states clear the disc, the path between them does not: K = 0 reports a free trajectory (dgp_traj_metrics' verdict), K = 7 a collision inside interval 0"""
  p, th, sdf = IC.motivating_case()
  _, c0, s0 = IO_.run(p, th, 0, sdf, 0.0)
  M, oe = MO.metrics(p, th, sdf, 0.0)
  assert s0[0, IO_.COL['in_coll']] == 0 and M[0, MO.COL['in_coll']] == 0 and not oe.any() and np.array_equal(c0, oe)
  d7, c7, s7 = IO_.run(p, th, 7, sdf, 0.0)
  assert d7.shape == (1, 17, 4) and s7[0, IO_.COL['in_coll']] == 1
  first, worst = int(s7[0, IO_.COL['first_colliding']]), int(s7[0, IO_.COL['worst_index']])
  assert 1 <= first <= 7 and 1 <= worst <= 7 and c7[0, worst] == s7[0, IO_.COL['max_penetration']] > 0.0
  assert not c7[0, 8:].any()                                                # the second interval is free
  assert s7[0, IO_.COL['num_colliding']] == np.count_nonzero(c7[0, 1:-1])


def _cfg(**kw):
  base = dict(num_states=64, dof=2, io_dtype=_capi.DGP_F32, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4,
              Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4)
  base.update(kw)
  return _capi.make_config(**base)


def test_entry_point_validates_arguments_without_gpu():
  """every call below fails validation, so nothing is launched"""
  api = _capi.get_api()
  assert 'gp_interpolate' in _capi.CApi.SYMBOLS and api.gp_interpolate is not None and api.abi_version() == _capi.DGP_ABI_VERSION
  s = _capi.Solver(_cfg())
  ok = s.sdf_arg(0x1000, 256, 256, 0)

  def code(*a, **kw):
    with pytest.raises(_capi.DgpError) as e:
      s.gp_interpolate(*a, **kw)
    assert len(str(e.value)) > 20
    return e.value.code
  assert code(0, 0x1000, 1, ok, th_dense=0x1000) == _capi.DGP_EINVAL and code(-3, 0x1000, 1, ok, th_dense=0x1000) == _capi.DGP_EINVAL      # batch
  assert code(8, 0x1000, -1, ok, th_dense=0x1000) == _capi.DGP_EINVAL and code(8, 0x1000, 1024, ok, th_dense=0x1000) == _capi.DGP_EINVAL  # num_inter
  assert b'num_inter' in api.last_error()
  assert code(8, None, 1, ok, th_dense=0x1000) == _capi.DGP_EINVAL                                          # th
  assert code(8, 0x1000, 1, ok) == _capi.DGP_EINVAL                                                        # no output at all
  assert code(8, 0x1000, 1, None, th_dense=0x1000, dense_cost=0x1000) == _capi.DGP_EINVAL                  # a cost output without sdf
  assert code(8, 0x1000, 1, None, summary=0x1000) == _capi.DGP_EINVAL                                      # a summary without sdf
  assert code(8, 0x1000, 1, s.sdf_arg(None, 256, 256, 0), summary=0x1000) == _capi.DGP_EINVAL              # ... or without sdf->data
  assert b'sdf' in api.last_error()
  assert api.gp_interpolate(None, 8, 0x1000, 1, ok, 0.0, 0x1000, None, None, None) == _capi.DGP_EINVAL     # handle
  s2 = _capi.Solver(_cfg(num_states=2))
  with pytest.raises(_capi.DgpError) as e:                                                                  # n = 2, K = 0: two dense states, no interior one
    s2.gp_interpolate(8, 0x1000, 0, ok, summary=0x1000)
  assert e.value.code == _capi.DGP_EINVAL and 'interior' in str(e.value)
  # a request of dgp_time_next_launch does not survive a rejected call
  assert api.time_next_launch(0x10, 0x20) == _capi.DGP_OK
  assert code(0, 0x1000, 1, ok, th_dense=0x1000) == _capi.DGP_EINVAL
  assert api.time_next_launch(None, None) == _capi.DGP_OK


def test_trampoline_argument_count_and_null_handle():
  pc = _capi.get_pycall()
  args = (0, 1, 0x1000, 1, 0x1000, 8, 8, 0, 0, 0, None, 0.0, 0x1000, None, None, 0)
  with pytest.raises(TypeError):
    pc.gp_interpolate(*args[:15])
  assert pc.gp_interpolate(*args) == _capi.DGP_EINVAL and b'null' in _capi.get_api().last_error()
  assert _capi.CtypesPycall(_capi.get_api()).gp_interpolate(*args) == _capi.DGP_EINVAL      # the ctypes stand-in takes the same positional arguments


def test_emulator_library_reports_the_entry_point_as_absent():
  api = harness.emul_api()
  assert api.gp_interpolate is None and api.gn_step is not None
  s = _capi.Solver(_cfg(), api=api)
  with pytest.raises(NotImplementedError, match='emul_gp_interpolate'):
    s.gp_interpolate(8, 0x1000, 1, th_dense=0x1000)


class RecordingPycall(object):
  def __init__(self): self.calls = []

  def gp_interpolate(self, *a):
    assert len(a) == 16, len(a)                                        # as csrc/dgp_pycall.c unpacks them
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


def test_interpolate_marshalling(layer):
  B, n, K = 3, 16, 4
  nd = (n - 1) * (K + 1) + 1
  th = torch.randn(B, n, 4, dtype=torch.float32, requires_grad=True)
  sdf = torch.randn(1, 1, 8, 10, dtype=torch.float32)
  # interpolation only: no grid goes down, no cost and no summary are asked for
  r = layer.interpolate(th, K)
  a = layer._pc.calls[-1]
  h = layer._solvers[torch.float32].h
  assert a[0] == h and a[1] == B and a[2] == th.data_ptr() and a[3] == K and a[4] is None
  assert a[11] == 0.0 and isinstance(a[11], float) and a[12] == r.th.data_ptr() and a[13] is None and a[14] is None and a[15] == 77
  assert r.th.shape == (B, nd, 4) and r.th.dtype == torch.float32 and not r.th.requires_grad and r.raw is None and r.cost is None and r.keys() == ()
  assert r.times.shape == (nd,) and r.times.dtype == torch.float64 and r.times[0] == 0 and abs(float(r.times[-1]) - 10.0) < 1e-12
  assert abs(float(r.times[K + 1]) - 10.0 / 15) < 1e-12 and abs(float(r.times[1]) - 10.0 / 15 / 5) < 1e-12
  with pytest.raises(AttributeError):
    r.in_collision
  # a shared (expand()ed) grid: stride 0, the summary
  r = layer.interpolate(th, K, sdf.expand(B, 1, 8, 10))
  a = layer._pc.calls[-1]
  assert a[4:11] == (sdf.data_ptr(), 8, 10, 0, _capi.DGP_SDF_ROWMAJOR, 0, None) and a[13] is None and a[14] == r.raw.data_ptr()
  assert r.raw.shape == (B, _capi.DGP_DENSE_COUNT) == (B, 6) and r.raw.dtype == torch.float64 and r.cost is None
  r.raw.copy_(torch.tensor([[0.0, 0.0, 0.0, 0.0, -1.0, 1.0], [1.0, 2.0, 0.25, 0.5, 7.0, 8.0], [1.0, 1.0, 0.125, 0.75, 3.0, 3.0]], dtype=torch.float64))
  assert r.in_collision.dtype == torch.bool and r.in_collision.tolist() == [False, True, True]
  for k, want in (('num_colliding', [0, 2, 1]), ('first_colliding', [-1, 7, 3]), ('worst_index', [1, 8, 3])):
    assert r[k].dtype == torch.int64 and r[k].tolist() == want and getattr(r, k).shape == (B,)
  assert r.avg_penetration.data_ptr() == r.raw[:, 2].data_ptr() and r.max_penetration.tolist() == [0.0, 0.5, 0.75]
  assert set(r.as_dict()) == {'in_collision', 'num_colliding', 'avg_penetration', 'max_penetration', 'first_colliding', 'worst_index'}
  with pytest.raises(AttributeError):
    r.no_such_column
  # per-sample grids, an epsilon, the raw costs
  per = torch.randn(B, 1, 8, 10, dtype=torch.float32)
  r = layer.interpolate(th, 0, per, eps=0.4, return_cost=True)
  a = layer._pc.calls[-1]
  assert a[3] == 0 and a[4:8] == (per.data_ptr(), 8, 10, 80) and a[11] == 0.4 and a[13] == r.cost.data_ptr()
  assert r.cost.shape == (B, n) and r.cost.dtype == torch.float32 and r.th.shape == (B, n, 4)
  # float64 trajectories get the float64 handle; a tiled grid goes down as tiles
  from dgpmp2_amd.utils.sdf_utils import tile_sdf
  t = tile_sdf(torch.randn(B, 1, 10, 13, dtype=torch.float64))
  r = layer.interpolate(th.detach().double(), 7, t)
  a = layer._pc.calls[-1]
  assert a[0] == layer._solvers[torch.float64].h and a[4:9] == (t.data_ptr(), 10, 13, 3 * 4 * 16, _capi.DGP_SDF_TILED4) and r.th.dtype == torch.float64
  # a non-contiguous trajectory tensor is made contiguous, not read with the wrong strides
  wide = torch.randn(B, n, 8, dtype=torch.float32)
  layer.interpolate(wide[:, :, :4], 1, per)
  assert layer._pc.calls[-1][2] != wide.data_ptr()
  for bad in (lambda: layer.interpolate(th[:, :5], 1, per), lambda: layer.interpolate(th, -1), lambda: layer.interpolate(th, 1024), lambda: layer.interpolate(th, 1.5),
              lambda: layer.interpolate(th, 1, return_cost=True), lambda: layer.interpolate(th, 1, torch.randn(2, 1, 8, 10))):
    with pytest.raises(ValueError):
      bad()
