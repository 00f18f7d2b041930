"""dgp_prior_samples without a GPU: tests/prior_oracle.py (the numpy restatement of include/dgpmp2_hip.h that tests/test_hip_prior.py holds the kernel against)
checked against the DEFINITION -- the covariance of its linear map z -> xi against the dense (A^T K^-1 A)^-1 of the start, goal and GP factors, its mean against the
dense solve and against one obstacle-free step of oracle/gpmp2_oracle --, the torch mirror utils.planner_utils.gp_prior_samples_torch against the oracle, the
generated normals, host-side argument validation of the entry point, and the marshalling of PlanLayer.prior_samples / sample_prior against a recording stand-in
for the trampoline.

The bounds.  The dense quantities are evaluated twice by one dtype-generic routine (Cholesky, forward substitution, V^T V), in float64 and in np.longdouble; `ref` is
the largest difference of the two relative to the largest entry: the dense reference's own error (its conditioning reaches 2e8).  The oracle is held to
max(10 x ref, FLOOR_EPS x eps), against the float64 AND against the longdouble reference.  A floor is needed because ref falls below eps where the dense system is
tiny and well conditioned (n = 2: 5e-17) while the oracle still rounds: on the path from z to one entry of xi lie about 64 roundings (whitening with L_c 5, two scans
of 6 levels with the dt v term 15, the two d-term rows of S^-1 and the lane's W 35, Matheron's subtraction and the output 3, the coefficients of P 6), an entry of
M M^T has two such factors, and the difference x - W y is formed from terms of the size of the unconditioned chain: FLOOR_EPS = 256 = 2 x 2 x 64, no term that grows with
a condition number.  Measured over every case below: the oracle stays within 2.4e-14 (110 eps) of the longdouble reference, covariance and mean, relative to the largest
entry, while ref runs from 5e-17 (n = 2) to 4e-11 (n = 64)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import prior_cases as PC_
import prior_oracle as PO
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2 import plan_layer as PL
from dgpmp2_amd.robot_models import PointRobot2D
from dgpmp2_amd.utils import planner_utils as PU
from oracle import gpmp2_oracle as O

EPS = np.finfo(np.float64).eps
KS = (1e-3, 0.01, 0.5)


# ---- the dense definition, in any floating type -------------------------------------------------------------------------------------------------------------------
def dense_system(p, T, th=None, start=None, goal=None):
  """-> (Lambda = A^T K^-1 A, R) of the start prior, the n - 1 GP factors and the goal prior in dtype T.  th None: R is the right-hand side whose solution is the
  mean (Lambda mu = R); th (n,d): R = A^T K^-1 b of a Gauss-Newton step from th (Lambda dtheta = R), the residuals formed in T."""
  n, dof, d = p.n, p.dof, p.state_dim
  dt = T(p.total_time_sec) / T(n - 1)
  Qci = np.asarray(p.Q_c_inv).astype(T)
  I, Z, Id = np.eye(dof, dtype=T), np.zeros((dof, dof), dtype=T), np.eye(d, dtype=T)
  Phi = np.block([[I, dt * I], [Z, I]])
  Qi = np.block([[T(12) / dt ** 3 * Qci, T(-6) / dt ** 2 * Qci], [T(-6) / dt ** 2 * Qci, T(4) / dt * Qci]])
  ws, wg = T(1) / T(p.K_s) ** 2, T(1) / T(p.K_g) ** 2
  L, R = np.zeros((n * d, n * d), dtype=T), np.zeros(n * d, dtype=T)
  L[:d, :d] += ws * Id
  L[-d:, -d:] += wg * Id
  J = np.concatenate([-Phi, Id], axis=1)
  JQ = J.T @ Qi
  for i in range(n - 1): L[i * d:(i + 2) * d, i * d:(i + 2) * d] += JQ @ J
  s, g = np.asarray(start).reshape(d).astype(T), np.asarray(goal).reshape(d).astype(T)
  if th is None:
    R[:d], R[-d:] = ws * s, wg * g
  else:
    x = np.asarray(th).astype(T)
    R[:d] += ws * (s - x[0])
    R[-d:] += wg * (g - x[-1])
    for i in range(n - 1): R[i * d:(i + 2) * d] -= JQ @ (x[i + 1] - Phi @ x[i])
  return L, R


def spd_inverse(A):
  N = A.shape[0]
  G = np.zeros_like(A)
  for j in range(N):
    G[j, j] = np.sqrt(A[j, j] - G[j, :j] @ G[j, :j])
    G[j + 1:, j] = (A[j + 1:, j] - G[j + 1:, :j] @ G[j, :j]) / G[j, j]
  V, E = np.zeros_like(A), np.eye(N, dtype=A.dtype)
  for i in range(N): V[i] = (E[i] - G[i, :i] @ V[:i]) / G[i, i]
  return V.T @ V


def rel(a, b): return float(np.abs(a - b).max() / np.abs(b).max())


FLOOR_EPS = 256      # module docstring


def bound(ref): return max(10 * ref, FLOOR_EPS * EPS)


def floor(p): return 4 * p.state_dim * EPS * np.linalg.cond(np.linalg.inv(np.array(PO.Consts(p).Sinv)))      # the torch mirror's bound only: it forms W_k through torch.linalg.inv


def random_spd(dof, seed):
  R = np.random.RandomState(seed).randn(dof, dof)
  Q = R @ R.T + dof * np.eye(dof)
  return (Q + Q.T) / 2


@pytest.mark.parametrize('n', [2, 3, 8, 64])
@pytest.mark.parametrize('dof', [2, 3])
def test_oracle_against_the_definition(dof, n):
  """Cov(xi) = M M^T of the oracle's linear map against the dense (A^T K^-1 A)^-1, and mu against the dense solve, within max(10 x ref, 256 eps) of the float64 and of
  the longdouble evaluation (module docstring).  Measured: the oracle within 2.4e-14 (110 eps) of the longdouble reference in every case; ref 5e-17 .. 4e-11."""
  rs = np.random.RandomState(100 * dof + n)
  worst = 0.0
  for ks in KS:
    for kg in KS:
      for name, Q in (('diagonal', np.diag(0.7 * np.arange(1, dof + 1))), ('random SPD', random_spd(dof, dof))):
        p = PC_.params(dof, n, Q, K_s=ks, K_g=kg)
        start, goal = rs.uniform(-4, 4, (1, 1, 2 * dof)), rs.uniform(-4, 4, (1, 1, 2 * dof))
        M = PO.linear_map(p)
        C_, mu = M @ M.T, PO.mu(p, start, goal)[0].reshape(-1)
        L64, R64 = dense_system(p, np.float64, None, start, goal)
        Lld, Rld = dense_system(p, np.longdouble, None, start, goal)
        S64, Sld = spd_inverse(L64), spd_inverse(Lld)
        m64, mld = S64 @ R64, Sld @ Rld
        ref_c, ref_m = rel(S64, Sld), rel(m64, mld)
        got = dict(cov64=rel(C_, S64), covld=rel(C_, Sld), mu64=rel(mu, m64), muld=rel(mu, mld))
        worst = max(worst, got['covld'], got['muld'])
        print('dof %d n %2d K_s %g K_g %g %s: covariance %.2e / %.2e against float64 / longdouble (ref %.2e), mean %.2e / %.2e (ref %.2e)' %
              (dof, n, ks, kg, name, got['cov64'], got['covld'], ref_c, got['mu64'], got['muld'], ref_m))
        assert got['cov64'] <= bound(ref_c) and got['covld'] <= bound(ref_c), (dof, n, ks, kg, name, got, ref_c)
        assert got['mu64'] <= bound(ref_m) and got['muld'] <= bound(ref_m), (dof, n, ks, kg, name, got, ref_m)
  print('worst distance to the longdouble reference: %.2e (%.0f eps)' % (worst, worst / EPS))


@pytest.mark.parametrize('dof,n,qc', [(2, 8, 'diag'), (3, 8, 'full'), (2, 64, 'full'), (3, 64, 'diag')])
def test_mean_against_one_obstacle_free_step_of_the_existing_oracle(dof, n, qc):
  """mu = th + dtheta of oracle.plan_layer_forward from an arbitrary th, far from every obstacle, with reg = 0 (the smallest the oracle accepts: its normal
  equations are SPD without it).  The bound, derived the same way: the same step evaluated by dense_system / spd_inverse in float64 and longdouble, ref their
  difference, max(10 x ref, 256 eps).  Measured: |mu - (th + dtheta)| 7e-15 .. 7e-11 with ref 1e-14 .. 1e-10 (the step from an arbitrary th weights residuals of order
  1e6 into R; the direct solve for mu does not); mu against the longdouble step 5e-16 .. 5e-14."""
  p = PC_.params(dof, n, qc, reg=0.0)
  rs = np.random.RandomState(7 * n + dof)
  start, goal, th, _ = PC_.inputs(dof, n, 1, 1, 3)
  th = rs.uniform(-3, 3, (1, n, 2 * dof))
  sdf = np.full((1, 1, 16, 16), 50.0)      # every state far from any obstacle: the obstacle rows of the system vanish
  qc_, ow, eps = p.static_covs(1)
  dth = O.plan_layer_forward(th, start, goal, sdf, qc_, ow, eps, p)[0]
  got = (th + dth)[0]
  steps = []
  for T in (np.float64, np.longdouble):
    L, R = dense_system(p, T, th[0], start, goal)
    steps.append(th[0].astype(T) + (spd_inverse(L) @ R).reshape(n, 2 * dof))
  ref = rel(steps[0], steps[1])
  want = PO.mu(p, start, goal)[0]
  e = rel(got, want)
  print('dof %d n %d %s: |mu - (th + dtheta)| %.2e, ref %.2e; mu against the longdouble step %.2e' % (dof, n, qc, e, ref, rel(want, steps[1])))
  assert e <= bound(ref)
  assert rel(want, steps[1]) <= bound(ref)


@pytest.mark.parametrize('dof,n', [(2, 3), (2, 17), (3, 65), (2, 130)])
def test_torch_mirror_equals_the_oracle(dof, n):
  """the mirror sums with cumsum (another association order) and forms W_k as matrices: equal to the oracle within eps (n + 4 d cond(S)) X, X the largest entry of
  the unconditioned chain plus the largest output -- n roundings of partial sums of at most X, and the product with S^-1"""
  for qc in ('diag', 'full'):
    p = PC_.params(dof, n, qc, K_s=0.05, K_g=0.02)
    B, S = 3, 4
    start, goal, mean, z = PC_.inputs(dof, n, B, S, n)
    k = PO.Consts(p)
    for m, scale in ((None, 0.7), (mean, 1.0), (None, 0.0)):
      want = PO.run(p, start, goal, z, m, scale)[0]
      got = PU.gp_prior_samples_torch(torch.from_numpy(start), torch.from_numpy(goal), torch.from_numpy(z), p.total_time_sec, n - 1, p.Q_c_inv, p.K_s, p.K_g,
                                      None if m is None else torch.from_numpy(m), scale)
      X = np.abs(PO.chain(k, z)).max() + np.abs(want).max()
      bd = EPS * (n + floor(p) / EPS) * X
      assert got.shape == (B, S, n, 2 * dof) and got.dtype == torch.float64
      assert np.abs(got.numpy() - want).max() <= bd, (dof, n, qc, scale, np.abs(got.numpy() - want).max(), bd)
    g32 = PU.gp_prior_samples_torch(torch.from_numpy(start).float(), torch.from_numpy(goal).float(), torch.from_numpy(z).float(), p.total_time_sec, n - 1, p.Q_c_inv,
                                    p.K_s, p.K_g)
    assert g32.dtype == torch.float32 and np.abs(g32.numpy() - PO.run(p, start, goal, z)[0]).max() < 1e-6 * (n + floor(p) / EPS) * X
  with pytest.raises(ValueError):
    PU.gp_prior_samples_torch(torch.zeros(1, 1, 4), torch.zeros(1, 1, 4), torch.zeros(1, 1, 9, 4), 10.0, 9, np.eye(2), 0.01, 0.01)


def test_scale_zero_is_the_mean_and_samples_differ():
  p = PC_.params(2, 17, 'full')
  start, goal, mean, z = PC_.inputs(2, 17, 2, 3, 5)
  assert np.array_equal(PO.run(p, start, goal, z, mean, 0.0)[0], np.broadcast_to(mean[:, None], (2, 3, 17, 4)))
  th = PO.run(p, start, goal, z, None, 1.0)[0]
  assert np.array_equal(PO.run(p, start, goal, z, None, 0.0)[0][:, 0], PO.mu(p, start, goal)) and not np.array_equal(th[:, 0], th[:, 1])
  # the samples are anchored: the end states stay within a few K_s / K_g of the start and the goal
  assert np.abs(th[:, :, 0] - start).max() < 6 * p.K_s and np.abs(th[:, :, -1] - goal).max() < 6 * p.K_g
  # a trajectory is a function of its own noise block alone
  z2 = z.copy(); z2[1, 2] += 1.0
  th2 = PO.run(p, start, goal, z2, None, 1.0)[0]
  assert np.array_equal(th2[0], th[0]) and np.array_equal(th2[1, :2], th[1, :2]) and not np.array_equal(th2[1, 2], th[1, 2])
  # info: bit 0 a position outside the limits, bit 1 a non-finite value
  far = PO.run(p, start, goal, z, None, 50.0)[1]
  assert far.shape == (2, 3) and (far == 1).all() and (PO.run(p, start, goal, z, None, 0.0)[1] == 0).all()
  zn = z.copy(); zn[0, 1, 4, 2] = np.nan
  clean = PO.run(p, start, goal, z, None, 1.0)[1]
  want = clean.copy(); want[0, 1] = 3
  assert np.array_equal(PO.run(p, start, goal, zn, None, 1.0)[1], want)      # the NaN reaches its own sample's flags and no other's


def test_scan_order_and_launch_choice():
  rs = np.random.RandomState(0)
  for n in (1, 2, 3, 17, 64, 65, 130, 257):
    e = rs.randn(2, n)
    s = PO.scan(e)
    np.testing.assert_allclose(s, np.cumsum(e, -1), rtol=0, atol=1e-13 * n)
    # the order is a function of the index alone: a longer array has the same prefix, bit for bit
    assert np.array_equal(PO.scan(np.concatenate([e, rs.randn(2, 70)], -1))[:, :n], s)
  assert [PO.lpt(n) for n in (2, 16, 17, 32, 33, 64, 65, 1024)] == [16, 16, 32, 32, 64, 64, 64, 64]
  assert [PO.is_long(n) for n in (2, 64, 65, 257)] == [False, False, True, True]
  # by hand: index 3 is (e0 + e1) + (e2 + e3), index 2 is e0 + (e1 + e2)
  e = np.array([0.1, 0.2, 0.3, 0.4])
  assert PO.scan(e)[3] == (0.1 + 0.2) + (0.3 + 0.4) and PO.scan(e)[2] == 0.1 + (0.2 + 0.3) != (0.1 + 0.2) + 0.3


NORMAL_SEED = 0


def test_generated_normals():
  """counters of different (problem, sample) never coincide; over all N normals of NORMAL_SEED (8 problems x 16 samples x 65 rows x 4):
  |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N)"""
  seen = set()
  for problem in (0, 1, 2, (1 << 32) + 1, (1 << 63) + 5):
    for s in (0, 1, 2, PO.MAX_SAMPLES - 1):
      c = set(PO.counters(problem, s, 17, 4))
      assert len(c) == 18 * 2 and not (c & seen)
      assert all(w[3] >> 24 == PO.STREAM_TAG and w[3] & 0xffffff == s for w in c)      # a stream of its own: dgp_sample_problems uses 0 / 1, dgp_obstacle_maps 0 .. 63 and 0xffffffff
      seen |= c
  z = PO.all_normals(NORMAL_SEED, 0, 8, 16, 64, 4)
  N = z.size
  assert z.shape == (8, 16, 65, 4) and N == 33280 and np.isfinite(z).all()
  print('mean %.4f (bound %.4f), var - 1 %.4f (bound %.4f)' % (z.mean(), 5 / np.sqrt(N), z.var() - 1, 5 * np.sqrt(2.0 / N)))
  assert abs(z.mean()) <= 5 / np.sqrt(N) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / N)
  # a block is a function of (seed, problem, s) alone, and another seed, problem or sample gives other normals
  assert np.array_equal(PO.normals(NORMAL_SEED, 3, 5, 64, 4), z[3, 5]) and np.array_equal(PO.all_normals(NORMAL_SEED, 2, 2, 3, 64, 4), z[2:4, :3])
  assert not np.array_equal(PO.normals(NORMAL_SEED + 1, 3, 5, 64, 4), z[3, 5]) and not np.array_equal(z[3, 4], z[3, 5]) and not np.array_equal(z[2, 5], z[3, 5])
  # the first normals of a shorter trajectory are those of a longer one (row-major blocks)
  assert np.array_equal(PO.normals(NORMAL_SEED, 3, 5, 8, 4).ravel(), z[3, 5].ravel()[:36])


def test_host_constants():
  for dof in (2, 3):
    k = PO.Consts(PC_.params(dof, 17, 'full', K_s=0.05, K_g=0.02))
    Q, L = np.array(k.Qc), np.array(k.Lc)
    np.testing.assert_allclose(Q @ PC_.QC_FULL[dof], np.eye(dof), atol=1e-15)
    np.testing.assert_allclose(L @ L.T, Q, atol=1e-16)
    assert np.array_equal(Q, Q.T) and np.array_equal(np.triu(L, 1), np.zeros((dof, dof)))
    assert abs(k.cp ** 2 - k.dt ** 3 / 3) < 1e-15 and abs(k.cp * k.cv1 - k.dt ** 2 / 2) < 1e-15 and abs(k.cv1 ** 2 + k.cv2 ** 2 - k.dt) < 1e-15
    assert np.array_equal(np.array(k.Sinv), np.array(k.Sinv).T)
  for bad in ([[1.0, 2.0], [2.0, 1.0]], [[1.0, 0.5], [0.25, 1.0]], [[0.0, 0.0], [0.0, 1.0]], [[np.nan, 0.0], [0.0, 1.0]]):
    with pytest.raises(ValueError):
      PO.Consts(PC_.params(2, 8, np.array(bad)))


# ---- the entry point, without a GPU -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def api():
  if not os.path.exists(_capi.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _capi.get_api()


def _cfg(**kw):
  base = dict(num_states=16, dof=2, io_dtype=_capi.DGP_F64, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4,
              Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4)
  base.update(kw)
  return _capi.make_config(**base)


def test_symbol_and_abi(api):
  assert 'prior_samples' in _capi.CApi.SYMBOLS and api.prior_samples is not None and api.abi_version() == 7 and _capi.DGP_ABI_VERSION == 7
  assert 'prior_samples' in _capi._PYCALL_ENTRIES and _capi.DGP_MAX_PRIOR_SAMPLES == PO.MAX_SAMPLES == 1 << 24
  assert 'prior_launch_shape' in _capi.CApi.SYMBOLS and api.prior_launch_shape is not None
  for n, want in ((2, (16, 1)), (16, (16, 1)), (17, (32, 1)), (32, (32, 1)), (33, (64, 1)), (64, (64, 1)), (65, (64, 2)), (128, (64, 2)), (129, (64, 3)), (1024, (64, 16))):
    assert _capi.Solver(_cfg(num_states=n)).prior_launch_shape() == want == (PO.lpt(n), (n + 63) // 64), n
  assert api.prior_launch_shape(None, None, None) == _capi.DGP_EINVAL and api.prior_launch_shape(_capi.Solver(_cfg()).handle, None, None) == _capi.DGP_OK


def test_prior_samples_validates_arguments_without_gpu(api):
  s = _capi.Solver(_cfg())
  call = lambda solver, batch=8, S=4, start=0x1000, goal=0x1000, th=0x1000, **kw: solver.prior_samples(batch, S, start, goal, th, **kw)

  def refused(*a, **kw):
    with pytest.raises(_capi.DgpError) as e:
      call(*a, **kw)
    assert len(str(e.value)) > 20 and e.value.code == _capi.DGP_EINVAL
    return e.value
  for kw in (dict(start=None), dict(goal=None), dict(th=None)): refused(s, **kw)
  for bad in (0, -2): assert 'batch' in str(refused(s, batch=bad))
  for bad in (0, -1, (1 << 24) + 1): assert 'num_samples' in str(refused(s, S=bad)), bad
  assert 'trajectories' in str(refused(s, batch=1 << 20, S=1 << 12))      # batch * num_samples past one launch
  for bad in (-1e-300, -1.0, float('nan'), float('inf'), -float('inf')): assert 'scale' in str(refused(s, scale=bad)), bad
  for q in ([[1, 2], [2, 1]], [[1, 0.5], [0.25, 1]], [[0, 0], [0, 1]], [[-1, 0], [0, 1]], [[float('nan'), 0], [0, 1]], [[float('inf'), 0], [0, 1]]):
    assert 'Q_c_inv' in str(refused(_capi.Solver(_cfg(Q_c_inv=q)))), q
  assert 'Q_c_inv' in str(refused(_capi.Solver(_cfg(dof=3, Q_c_inv=[[1, 0, 0], [0, 1, 2], [0, 2, 1]]))))

  def raw(h, start=0x1000, goal=0x1000, th=0x1000):
    return api.prior_samples(h, 8, 4, start, goal, None, 1.0, 0, 0, None, th, None, None, None)
  assert raw(None) == _capi.DGP_EINVAL and b'null handle' in api.last_error()
  for kw in (dict(start=None), dict(goal=None), dict(th=None)): assert raw(s.handle, **kw) == _capi.DGP_EINVAL, kw
  # a request of dgp_time_next_launch does not survive a rejected call
  assert api.time_next_launch(0x10, 0x20) == _capi.DGP_OK
  assert raw(None) == _capi.DGP_EINVAL
  refused(s, batch=0)
  assert api.time_next_launch(None, None) == _capi.DGP_OK
  # the ctypes stand-in of the trampoline takes the same positional arguments
  assert _capi.CtypesPycall(api).prior_samples(s.h, 0, 4, 0x1000, 0x1000, None, 1.0, 0, 0, None, 0x1000, None, None, None) == _capi.DGP_EINVAL


def test_emulator_library_reports_the_entry_point_as_absent():
  import harness
  eapi = harness.emul_api()
  assert eapi.prior_samples is None and eapi.gn_step is not None
  with pytest.raises(NotImplementedError, match='emul_prior_samples'):
    _capi.Solver(_cfg(), api=eapi).prior_samples(8, 4, 0x1000, 0x1000, 0x1000)
  with pytest.raises(NotImplementedError, match='emul_prior_launch_shape'):
    _capi.Solver(_cfg(), api=eapi).prior_launch_shape()


class RecordingPycall(object):
  def __init__(self): self.calls = []

  def prior_samples(self, *a):
    assert len(a) == 14, len(a)                                        # as csrc/dgp_pycall.c unpacks them
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


class _FakeCuda(object):
  """a tensor that says it lives on the device: the argument checks are all that read it here"""

  def __new__(cls, *shape, **kw):
    class T(torch.Tensor):
      @property
      def is_cuda(self): return True
    return torch.zeros(*shape, **kw).as_subclass(T)


def test_prior_samples_marshalling(layer):
  B, S, n, d = 3, 5, 16, 4
  st, go = torch.randn(B, 1, d, dtype=torch.float32), torch.randn(B, 1, d, dtype=torch.float32)
  th, noise, info = layer.prior_samples(st, go, S)
  a = layer._pc.calls[-1]
  assert a[0] == layer._solvers[torch.float32].h and a[1:3] == (B, S) and a[3] == st.data_ptr() and a[4] == go.data_ptr() and a[5] is None
  assert a[6] == 1.0 and isinstance(a[6], float) and a[7:10] == (0, 0, None) and a[10] == th.data_ptr() and a[11] is None and a[12] == info.data_ptr() and a[13] == 77
  assert th.shape == (B, S, n, d) and th.dtype == torch.float32 and noise is None and info.shape == (B, S) and info.dtype == torch.int32
  # every option: a float64 handle for float32 inputs, a mean, a scale, a seed, supplied noise and the normals returned
  mean, z = torch.randn(B, n, d, dtype=torch.float64), torch.randn(B, S, n + 1, d, dtype=torch.float64)
  th, noise, info = layer.prior_samples(st, go, S, torch.float64, mean, 0.25, 9, 1 << 40, z, True)
  a = layer._pc.calls[-1]
  assert a[0] == layer._solvers[torch.float64].h and a[3] != st.data_ptr() and a[5] == mean.data_ptr() and a[6] == 0.25 and a[7:9] == (9, 1 << 40) and a[9] == z.data_ptr()
  assert a[11] == noise.data_ptr() and noise.shape == (B, S, n + 1, d) and noise.dtype == torch.float64 and th.dtype == torch.float64
  # a non-contiguous mean and float32 noise are converted, not read with the wrong strides / type
  wide = torch.randn(B, n, 2 * d, dtype=torch.float64)
  layer.prior_samples(st, go, S, torch.float64, wide[:, :, :d], noise=z.float())
  a = layer._pc.calls[-1]
  assert a[5] != wide.data_ptr() and a[9] != z.data_ptr() and a[9] is not None
  for bad in (lambda: layer.prior_samples(st, go, 0), lambda: layer.prior_samples(st, go, 2.5), lambda: layer.prior_samples(st, go, (1 << 24) + 1),
              lambda: layer.prior_samples(st, go[:, :, :2], S), lambda: layer.prior_samples(st, go[:2], S), lambda: layer.prior_samples(st, go, S, scale=-1.0),
              lambda: layer.prior_samples(st, go, S, scale=float('nan')), lambda: layer.prior_samples(st, go, S, mean=mean[:, :5]),
              lambda: layer.prior_samples(st, go, S, noise=z[:, :, :n]), lambda: layer.prior_samples(st, go, S, noise=z[:, :2])):
    with pytest.raises(ValueError):
      bad()
  with pytest.raises(TypeError):
    layer.prior_samples(st.half(), go.half(), S)


def test_sample_prior_front_end(layer):
  from dgpmp2_amd import datasets as D
  from dgpmp2_amd.datasets import problem_generation as PG
  assert D.prior_samples is PG.prior_samples and D.PriorSampleInfo is PG.PriorSampleInfo
  z4 = torch.zeros(2, 1, 4)
  with pytest.raises(RuntimeError, match='startb.*CUDA/ROCm'):
    PG.prior_samples(layer, z4, z4, 3)
  with pytest.raises(RuntimeError, match='mean.*CUDA/ROCm'):
    PG.prior_samples(layer, _FakeCuda(2, 1, 4), _FakeCuda(2, 1, 4), 3, mean=torch.zeros(2, 16, 4))
  st, go = _FakeCuda(2, 1, 4, dtype=torch.float64), _FakeCuda(2, 1, 4, dtype=torch.float64)
  th, info = layer.sample_prior(st, go, 3, seed=11, first_problem=5, scale=0.5, return_noise=True)
  a = layer._pc.calls[-1]
  assert a[1:3] == (2, 3) and a[6:9] == (0.5, 11, 5) and a[9] is None and a[10] == th.data_ptr() and a[11] == info.noise.data_ptr() and a[12] == info.flags.data_ptr()
  assert isinstance(info, PG.PriorSampleInfo) and th.shape == (2, 3, 16, 4) and th.dtype == torch.float64 and info.noise.shape == (2, 3, 17, 4)
  th, info = PG.prior_samples(layer, st, go, 3, dtype=torch.float32)
  assert th.dtype == torch.float32 and info.noise is None and layer._pc.calls[-1][0] == layer._solvers[torch.float32].h
  flags = PG.PriorSampleInfo(torch.tensor([[0, 1], [2, 3]], dtype=torch.int32))
  assert flags.outside_limits.tolist() == [[False, True], [False, True]] and flags.non_finite.tolist() == [[False, False], [True, True]] and flags.noise is None
  # the planner's method is the same call
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner

  class P(object):
    plan_layer = layer
  th, info = DiffGPMP2Planner.sample_prior(P(), st, go, 4, seed=2)
  assert th.shape == (2, 4, 16, 4) and layer._pc.calls[-1][7] == 2
