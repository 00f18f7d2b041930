"""CPU-only tests of the training-loss feature (dgp_step_loss / dgp_step_loss_backward and what sits on top of them): the numpy oracle of include/dgpmp2_hip.h
(tests/loss_oracle.py) and the torch mirror utils.learn_utils.one_step_loss_torch against fixture g12_step_loss (the reference's own one_step_loss and autograd), the
column rule for dof 3, host-side argument validation of both entry points, and the marshalling of planner.step_loss / learn_utils.one_step_loss against a recording
stand-in for the trampoline.  The kernels themselves: tests/test_hip_loss.py (-m gpu).

Bounds.  A term is a sum of N non-negative addends, then at most 8 roundings (a division, the weighted combinations): any two summation orders agree to
(N + 8) 2^-53 relative (loss_oracle.sum_bound); against the fixture, whose sums run in yet another order, twice that.  A gradient is one product of the miss with a
factor formed by at most 4 operations: 8 x 2^-53 relative per element."""
import numpy as np
import pytest
import torch

import harness
import loss_cases as LC
import loss_oracle as LO
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2 import plan_layer as PL
from dgpmp2_amd.robot_models import PointRobot2D
from dgpmp2_amd.utils import learn_utils as LU

GRAD_TOL = 8 * LO.U


def fixture_cases(g):
  for B, n in g['shapes'].tolist():
    pre = 'B%d_n%d_' % (B, n)
    c = {k: g[pre + k] for k in ('update', 'target', 'target_sub', 'sg', 'gp', 'obs')}
    for wi, w in enumerate(g['weights'].tolist()):
      yield B, n, c, tuple(w), {k: g['%sw%d_%s' % (pre, wi, k)] for k in ('terms', 'g_update', 'g_target_sub', 'g_sg', 'g_gp', 'g_obs')}


def term_addends(B, n, dof=2):
  """number of addends behind each of the eight terms (EXT and TOTAL: the largest of their parts)"""
  e, s = B * n * dof, B
  return np.array([e, e, e, 1, s, s, s, s])


def terms_close(got, want, B, n, factor=1.0, dof=2):
  bound = factor * (term_addends(B, n, dof) + 8) * LO.U
  err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
  err[got == want] = 0.0
  return bool((err <= bound).all()), err / bound


def grads_close(got, want, tol=GRAD_TOL):
  got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
  err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
  err[got == want] = 0.0
  return bool((err <= tol).all())


def test_fixture_shape(golden):
  g = golden('g12_step_loss')
  assert g['shapes'].tolist() == [[1, 2], [3, 16], [5, 17], [7, 33]] and g['weights'].tolist() == [list(w) for w in LC.WEIGHTS] and float(g['cotangent']) == 0.5
  for B, n, c, w, ref in fixture_cases(g):
    regenerated = LC.mixed_batch(2, n, B)
    assert all(np.array_equal(c[k], regenerated[k]) for k in c), (B, n)      # the tests' generator is the fixture's
    assert ref['terms'].shape == (8,) and ref['terms'][LO.COL['cov']] == 0.0 and ref['g_update'].shape == (B, n, 4) and ref['g_sg'].shape == (B,)
    if B >= 5:
      m = LO.miss(c['update'], c['target'], c['target_sub'])
      assert not m[0].any() and np.abs(m[1]).max() > 512 and not c['sg'][2] and np.abs(m[3]).max() < 16      # exact hit, large, zero errors, ordinary


def test_oracle_against_the_reference(golden):
  g = golden('g12_step_loss')
  for B, n, c, w, ref in fixture_cases(g):
    terms, per = LO.forward(c['update'], c['target'], c['target_sub'], c['sg'], c['gp'], c['obs'], w, 2)
    ok, frac = terms_close(terms, ref['terms'], B, n, factor=2.0)
    print('B %d n %d w %s: terms at %s of the bound' % (B, n, w, np.round(frac, 3).tolist()))
    assert ok, (B, n, w, frac)
    assert per.shape == (B, 5) and LC.same_bits(per[:, 2:], np.stack([c['gp'], c['sg'], c['obs']], 1))
    gr = LO.backward(c['update'], c['target'], c['target_sub'], w, 2, g=float(g['cotangent']))
    for mine, theirs in (('update', 'g_update'), ('target_sub', 'g_target_sub'), ('sg', 'g_sg'), ('gp', 'g_gp'), ('obs', 'g_obs')):
      assert grads_close(gr[mine], ref[theirs]), (B, n, w, mine)
    assert LC.same_bits(gr['target'], -gr['update']) and LC.same_bits(gr['target_sub'], gr['update'])
    # the two-array form on the pre-formed difference: the same bits (the difference is exact for these inputs)
    two = LO.forward(c['update'], c['target'] - c['target_sub'], None, c['sg'], c['gp'], c['obs'], w, 2)
    assert LC.same_bits(two[0], terms) and LC.same_bits(two[1], per)


def test_torch_mirror_against_the_reference(golden):
  g = golden('g12_step_loss')
  T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
  for B, n, c, w, ref in fixture_cases(g):
    wd = dict(vel_loss_lambda=w[0], ext_obs_lambda=w[1], ext_loss_weight=w[2])
    dth, th_curr = T(c['update']).requires_grad_(True), T(c['target_sub']).requires_grad_(True)
    e = [T(c[k]).reshape(B, 1, 1).requires_grad_(True) for k in ('sg', 'gp', 'obs')]
    for form in ('two-array', 'three-array', 'reference signature'):
      if form == 'two-array': out = LU.one_step_loss_torch(dth, T(c['target']) - th_curr, *e, wd)
      elif form == 'three-array': out = LU.one_step_loss_torch(dth, T(c['target']), *e, wd, dof=2, target_sub=th_curr)
      else: out = LU.one_step_loss(dth, T(c['target']) - th_curr, None, None, *e, None, {'optim': wd}, 2, 0)
      assert len(out) == 8 and all(t.dim() == 0 and t.dtype == torch.float64 for t in out)
      terms = np.array([float(t.detach()) for t in out])
      ok, frac = terms_close(terms, ref['terms'], B, n, factor=2.0)
      assert ok, (form, B, n, w, frac)
      grads = torch.autograd.grad(float(g['cotangent']) * out[0], [dth, th_curr] + e)
      for got, name in zip(grads, ('g_update', 'g_target_sub', 'g_sg', 'g_gp', 'g_obs')):
        assert grads_close(got.numpy(), ref[name]), (form, B, n, w, name)
  # absent errors are zero terms
  out = [t.detach() for t in LU.one_step_loss_torch(dth, T(c['target']), None, None, None, wd)]
  assert float(out[4]) == float(out[5]) == float(out[6]) == float(out[7]) == 0.0 and float(out[0]) == float(out[1] + wd['vel_loss_lambda'] * out[2])


def test_columns_are_positions_then_velocities():
  rs = np.random.RandomState(5)
  w = (0.5, 2.0, 0.3)
  # dof 3: [0, 3) positions, [3, 6) velocities -- a miss in theta (column 2) is a position miss, one in omega (column 5) a velocity miss
  B, n = 3, 4
  z = np.zeros((B, n, 6))
  for col, hit, other in ((2, 'pos', 'vel'), (5, 'vel', 'pos'), (3, 'vel', 'pos'), (0, 'pos', 'vel')):
    u = z.copy(); u[:, :, col] = rs.randint(1, 9, (B, n))
    terms, per = LO.forward(u, z, None, None, None, None, w, 3)
    assert terms[LO.COL[hit]] == (u ** 2).sum() / (B * n) and terms[LO.COL[other]] == 0.0, col
    assert per[:, LO.PER_TRAJ.index(hit)].tolist() == (u ** 2).sum((1, 2)).tolist()
    gr = LO.backward(u, z, None, w, 3)
    k = 2.0 / (B * n) * (1.0 if hit == 'pos' else w[0])
    assert np.array_equal(gr['update'][:, :, col], u[:, :, col] * k) and not np.delete(gr['update'], col, 2).any()
    tt = LU.one_step_loss_torch(torch.from_numpy(u), torch.from_numpy(z), None, None, None, dict(zip(('vel_loss_lambda', 'ext_obs_lambda', 'ext_loss_weight'), w)), dof=3)
    assert float(tt[LO.COL[hit]]) == terms[LO.COL[hit]] and float(tt[LO.COL[other]]) == 0.0
  # dof 2: exactly the reference's hard-coded columns 0,1 / 2,3
  c = LC.mixed_batch(2, 17, 5)
  m = LO.miss(c['update'], c['target'], c['target_sub'])
  terms, per = LO.forward(c['update'], c['target'], c['target_sub'], c['sg'], c['gp'], c['obs'], w, 2)
  hard_pos = np.asarray(np.sum(np.asarray(m[:, :, [0, 1]] ** 2, np.longdouble).reshape(5, -1), 1), np.float64)
  hard_vel = np.asarray(np.sum(np.asarray(m[:, :, [2, 3]] ** 2, np.longdouble).reshape(5, -1), 1), np.float64)
  assert LC.same_bits(per[:, 0], hard_pos) and LC.same_bits(per[:, 1], hard_vel)
  assert {LO.lpt(n) for n in (1, 2, 3, 16, 17, 32, 33, 65, 130, 257)} == {16, 32, 64} and LO.lpt(16) == 16 and LO.lpt(17) == 32 and LO.lpt(33) == 64


def test_library_exports_the_entry_points():
  api = _capi.get_api()
  assert 'step_loss' in _capi.CApi.SYMBOLS and 'step_loss_backward' in _capi.CApi.SYMBOLS
  assert api.step_loss is not None and api.step_loss_backward is not None and api.abi_version() == _capi.DGP_ABI_VERSION == 7
  assert _capi.LOSS_NAMES == LO.NAMES and _capi.DGP_LOSS_COUNT == 8 and _capi.DGP_LOSS_PER_TRAJ == 5 == len(LO.PER_TRAJ) and _capi.LOSS_PER_TRAJ_NAMES == LO.PER_TRAJ
  assert [_capi.DGP_LOSS_TOTAL, _capi.DGP_LOSS_COV, _capi.DGP_LOSS_EXT] == [0, 3, 7] and LU.TERM_NAMES == LO.NAMES


def test_entry_points_validate_arguments_without_gpu():
  """every call below fails validation, so nothing is launched"""
  api = _capi.get_api()
  P, W = 0x1000, (0.5, 2.0, 0.3)
  F32, F64 = _capi.DGP_F32, _capi.DGP_F64

  def fwd(dtype=F32, B=8, n=16, dof=2, update=P, target=P, weights=W, terms=P, per_traj=P, **kw):
    with pytest.raises(_capi.DgpError) as e:
      _capi.step_loss(dtype, B, n, dof, update, target, weights, terms, per_traj, **kw)
    assert len(str(e.value)) > 20
    return e.value.code

  def bwd(dtype=F64, B=8, n=16, dof=3, update=P, target=P, weights=W, **kw):
    with pytest.raises(_capi.DgpError) as e:
      _capi.step_loss_backward(dtype, B, n, dof, update, target, weights, **kw)
    assert len(str(e.value)) > 20
    return e.value.code
  E = _capi.DGP_EINVAL
  nan = float('nan')
  for call, extra in ((fwd, {}), (bwd, dict(g_update=P))):
    assert call(dtype=_capi.DGP_U8, **extra) == E and call(dtype=7, **extra) == E and b'dtype' in api.last_error()
    assert call(B=0, **extra) == E and call(B=-2, **extra) == E and call(n=0, **extra) == E
    assert call(dof=1, **extra) == E and call(dof=4, **extra) == E and b'dof' in api.last_error()
    assert call(update=None, **extra) == E and call(target=None, **extra) == E and call(weights=None, **extra) == E
    for k in range(3):
      assert call(weights=tuple(nan if i == k else v for i, v in enumerate(W)), **extra) == E and b'NaN' in api.last_error()
  assert fwd(terms=None) == E and fwd(per_traj=None) == E and b'per_traj' in api.last_error()
  assert bwd() == E and bwd(g_total=P) == E and b'null' in api.last_error()                          # every output NULL
  # a request of dgp_time_next_launch does not survive a rejected call
  assert api.time_next_launch(0x10, 0x20) == _capi.DGP_OK
  assert fwd(B=0) == E and bwd() == E
  assert api.time_next_launch(None, None) == _capi.DGP_OK


def test_trampoline_argument_counts():
  pc = _capi.get_pycall()
  f = (_capi.DGP_F32, 0, 16, 2, 0x1000, 0x1000, None, None, None, None, 0.5, 2.0, 0.3, 0x1000, 0x1000, 0)                     # batch 0: rejected, nothing launched
  b = (_capi.DGP_F32, 0, 16, 2, 0x1000, 0x1000, None, 0.5, 2.0, 0.3, None, 0x1000, None, None, None, None, None, 0)
  with pytest.raises(TypeError):
    pc.step_loss(*f[:15])
  with pytest.raises(TypeError):
    pc.step_loss_backward(*b[:17])
  assert pc.step_loss(*f) == _capi.DGP_EINVAL and b'batch' in _capi.get_api().last_error()
  assert pc.step_loss_backward(*b) == _capi.DGP_EINVAL
  ct = _capi.CtypesPycall(_capi.get_api())      # the ctypes stand-in takes the same positional arguments
  assert ct.step_loss(*f) == _capi.DGP_EINVAL and ct.step_loss_backward(*b) == _capi.DGP_EINVAL


def test_emulator_library_reports_the_entry_points_as_absent():
  api = harness.emul_api()
  assert api.step_loss is None and api.step_loss_backward is None and api.gn_step is not None
  with pytest.raises(NotImplementedError, match='emul_step_loss'):
    _capi.step_loss(_capi.DGP_F32, 8, 16, 2, 0x1000, 0x1000, (0.5, 2.0, 0.3), 0x1000, 0x1000, api=api)
  with pytest.raises(NotImplementedError, match='emul_step_loss_backward'):
    _capi.step_loss_backward(_capi.DGP_F32, 8, 16, 2, 0x1000, 0x1000, (0.5, 2.0, 0.3), g_update=0x1000, api=api)


class RecordingPycall(object):
  def __init__(self): self.fwd, self.bwd = [], []

  def step_loss(self, *a):
    assert len(a) == 16, len(a)                                        # as csrc/dgp_pycall.c unpacks them
    self.fwd.append(a)
    return 0

  def step_loss_backward(self, *a):
    assert len(a) == 18, len(a)
    self.bwd.append(a)
    return 0


@pytest.fixture
def recorder(monkeypatch):
  monkeypatch.setattr(PL, '_require_cuda', lambda t, name: None)
  monkeypatch.setattr(PL, '_cur_dev', lambda: -1)
  monkeypatch.setattr(PL, '_raw_stream', lambda i: 77)
  return RecordingPycall()


@pytest.fixture
def layer(recorder):
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  n = 16
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  lp = {'optim': {'vel_loss_lambda': 0.5, 'ext_obs_lambda': 2.0, 'ext_loss_weight': 0.3}}
  pl = PL.PlanLayer(gp, ob, pp, op, {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}, PointRobot2D(t(0.4), 1, n))
  pl.learn_params = lp                                               # (only its 'optim' block is read: the default weights)
  pl.__dict__['_pc'] = recorder
  return pl


def test_step_loss_marshalling(layer):
  """planner.step_loss: the three-array form, the weights of learn_params['optim'], NULL for absent errors, the cotangent's address handed to the one backward call"""
  B, n = 3, 16
  pc = layer._pc
  dth = torch.randn(B, n, 4, dtype=torch.float32, requires_grad=True)
  th_curr = torch.randn(B, n, 4, dtype=torch.float32, requires_grad=True)
  th_opt = torch.randn(B, n, 4, dtype=torch.float32)
  e_sg, e_gp, e_obs = torch.rand(B, 1, requires_grad=True), torch.rand(B, 1, 1, requires_grad=True), torch.rand(B, 1, 1)
  r = layer.step_loss(dth, th_curr, th_opt, (e_sg, e_gp, e_obs))
  a = pc.fwd[-1]
  assert a[:4] == (_capi.DGP_F32, B, n, 2)
  assert a[4:7] == (dth.data_ptr(), th_opt.data_ptr(), th_curr.data_ptr())                          # update, target, target_sub
  assert a[7:10] == (e_sg.data_ptr(), e_gp.data_ptr(), e_obs.data_ptr())                            # unw_sg, unw_gp, unw_obs
  assert a[10:13] == (0.5, 2.0, 0.3) and all(isinstance(v, float) for v in a[10:13])
  assert a[13] == r.raw.data_ptr() and a[14] == r.per_sample.data_ptr() and a[15] == 77
  assert isinstance(r, PL.LossTerms) and r._fields == ('total', 'pos', 'vel', 'cov', 'gp', 'sg', 'obs', 'ext') == LO.NAMES
  assert r.raw.shape == (8,) and r.raw.dtype == torch.float64 and r.per_sample.shape == (B, 5) and r.per_sample.dtype == torch.float64
  for i, t in enumerate(r):
    assert t.dim() == 0 and t.dtype == torch.float64 and t.data_ptr() == r.raw.data_ptr() + 8 * i      # views of the one result: no cast kernels
  assert r.total.requires_grad and not any(t.requires_grad for t in r[1:]) and not r.raw.requires_grad and not r.per_sample.requires_grad
  # the backward: one call, fed the incoming cotangent's address; gradients for the inputs that require them only
  got = []
  r.total.register_hook(lambda g: got.append(g))
  (r.total * 0.5).backward()
  assert len(pc.bwd) == 1 and len(got) == 1 and got[0].dim() == 0 and got[0].dtype == torch.float64
  b = pc.bwd[-1]
  assert b[:4] == (_capi.DGP_F32, B, n, 2) and b[4:7] == (dth.data_ptr(), th_opt.data_ptr(), th_curr.data_ptr()) and b[7:10] == (0.5, 2.0, 0.3)
  assert b[10] == got[0].data_ptr() and float(got[0]) == 0.5
  assert b[11] is not None and b[12] is None and b[13] is not None                                   # g_update, no g_target (th_opt needs none), g_target_sub
  assert b[14] is not None and b[15] is not None and b[16] is None and b[17] == 77                   # g_unw_sg, g_unw_gp, no g_unw_obs
  assert dth.grad.shape == dth.shape and th_curr.grad.shape == th_curr.shape and e_sg.grad.shape == (B, 1) and e_gp.grad.shape == (B, 1, 1) and th_opt.grad is None
  with pytest.raises(RuntimeError):                                                                   # once differentiable
    torch.autograd.grad(torch.autograd.grad(layer.step_loss(dth, th_curr, th_opt, (e_sg, e_gp, e_obs)).total, dth, create_graph=True)[0].sum(), dth)
  # absent errors go down as NULL; explicit weights; float64 inputs; a non-contiguous update is made contiguous
  wide = torch.randn(B, n, 8, dtype=torch.float64)
  r = layer.step_loss(wide[:, :, :4], th_curr.detach().double(), th_opt.double(), (None, e_gp.detach().double(), None), weights=dict(vel_loss_lambda=0, ext_obs_lambda=1, ext_loss_weight=torch.tensor(1.0)))
  a = pc.fwd[-1]
  assert a[0] == _capi.DGP_F64 and a[4] != wide.data_ptr() and a[7] is None and a[8] is not None and a[9] is None and a[10:13] == (0.0, 1.0, 1.0)
  assert not r.total.requires_grad
  for bad in (lambda: layer.step_loss(dth[:, :5], th_curr, th_opt, (e_sg, e_gp, e_obs)), lambda: layer.step_loss(dth, th_curr[:2], th_opt, (e_sg, e_gp, e_obs)),
              lambda: layer.step_loss(dth, th_curr, th_opt, (e_sg[:2], e_gp, e_obs))):
    with pytest.raises(ValueError):
      bad()
  layer.learn_params = None
  with pytest.raises(ValueError):
    layer.step_loss(dth, th_curr, th_opt, (e_sg, e_gp, e_obs))


def test_one_step_loss_marshalling(recorder, monkeypatch):
  """learn_utils.one_step_loss on device tensors: the reference's signature, the two-array form (target_sub NULL), dof as given"""
  monkeypatch.setattr(_capi, '_pycall', recorder)
  monkeypatch.setattr(LU, '_on_device', lambda t: True)
  B, n = 4, 9
  lp = {'optim': {'vel_loss_lambda': 0.25, 'ext_obs_lambda': 1.5, 'ext_loss_weight': 0.75}}
  for dof in (2, 3):
    dth = torch.randn(B, n, 2 * dof, dtype=torch.float64, requires_grad=True)
    th_curr = torch.randn(B, n, 2 * dof, dtype=torch.float64, requires_grad=True)
    target = torch.randn(B, n, 2 * dof, dtype=torch.float64) - th_curr
    e_sg, e_gp, e_obs = torch.rand(B, 1, dtype=torch.float64), torch.rand(B, 1, 1, dtype=torch.float64), torch.rand(B, 1, 1, dtype=torch.float64)
    out = LU.one_step_loss(dth, target, None, None, e_sg, e_gp, e_obs, None, lp, dof, 3)
    a = recorder.fwd[-1]
    assert len(out) == 8 and all(t.dim() == 0 and t.dtype == torch.float64 for t in out)
    assert a[:4] == (_capi.DGP_F64, B, n, dof) and a[4] == dth.data_ptr() and a[5] == target.data_ptr() and a[6] is None
    assert a[7:10] == (e_sg.data_ptr(), e_gp.data_ptr(), e_obs.data_ptr()) and a[10:13] == (0.25, 1.5, 0.75) and a[15] == 77
    out[0].backward()
    b = recorder.bwd[-1]
    assert b[6] is None and b[10] is not None and b[11] is not None and b[12] is not None and b[13] is None and b[14:17] == (None, None, None)
    assert dth.grad is not None and th_curr.grad is not None                                         # (through autograd's own subtraction node)
