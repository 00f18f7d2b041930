"""numpy restatement of dgp_step_loss / dgp_step_loss_backward (include/dgpmp2_hip.h): per-element operations in the header's order in float64, sums in
np.longdouble in index order, gradients in the header's operation order.  For fp32 I/O it is fed the fp32-exact inputs and rounds every stored value once.
Shared by tests/test_loss_oracle.py (CPU) and tests/test_hip_loss.py (GPU)."""
import numpy as np

NAMES = ('total', 'pos', 'vel', 'cov', 'gp', 'sg', 'obs', 'ext')
COL = {k: i for i, k in enumerate(NAMES)}
PER_TRAJ = ('pos', 'vel', 'gp', 'sg', 'obs')
U = 2.0 ** -53


def lpt(n):
  """lanes per trajectory of the first forward launch (csrc/step_loss.hip: rows_lpt)"""
  return 16 if n <= 16 else 32 if n <= 32 else 64


def rnd(a, io):
  """a float64 array holding values exactly representable in the I/O type"""
  return None if a is None else (np.asarray(a, np.float64) if io == 'f64' else np.asarray(a, np.float32).astype(np.float64))


def miss(update, target, target_sub=None):
  u, t = np.asarray(update, np.float64), np.asarray(target, np.float64)
  return u - t if target_sub is None else u - (t - np.asarray(target_sub, np.float64))


def _sum(a, axis=None):
  """index-order sum in extended precision, rounded once"""
  return np.asarray(np.sum(np.asarray(a, np.longdouble), axis=axis), np.float64)


def per_traj(update, target, target_sub, sg, gp, obs, dof):
  """(B, 5): pos_b, vel_b, gp_b, sg_b, obs_b"""
  m = miss(update, target, target_sub)
  B = m.shape[0]
  sq = m * m
  e = lambda a: np.zeros(B) if a is None else np.asarray(a, np.float64).reshape(B)
  return np.stack([_sum(sq[:, :, :dof].reshape(B, -1), 1), _sum(sq[:, :, dof:2 * dof].reshape(B, -1), 1), e(gp), e(sg), e(obs)], 1)


def terms_from(per, n, w):
  """(8,) from the (B, 5) per-trajectory array; w = (vel_loss_lambda, ext_obs_lambda, ext_loss_weight)"""
  B = per.shape[0]
  s = _sum(per, 0)
  fb, fbn = float(B), float(B) * float(n)
  pos, vel, gp, sg, obs = s[0] / fbn, s[1] / fbn, s[2] / fb, s[3] / fb, s[4] / fb
  ext = (gp + sg) + w[1] * obs
  total = (pos + w[0] * vel) + w[2] * ext
  return np.array([total, pos, vel, 0.0, gp, sg, obs, ext])


def forward(update, target, target_sub, sg, gp, obs, w, dof):
  """-> terms (8,), per_traj (B, 5)"""
  per = per_traj(update, target, target_sub, sg, gp, obs, dof)
  return terms_from(per, np.asarray(update).shape[1], w), per


def backward(update, target, target_sub, w, dof, g=1.0, io='f64'):
  """-> dict(update, target, target_sub (B,n,d), sg, gp, obs (B)): every gradient in the header's operation order, rounded once to the I/O type"""
  m = miss(update, target, target_sub)
  B, n, d = m.shape
  g = float(g)
  fb, fbn = float(B), float(B) * float(n)
  c_ext = w[2] * g
  k_pos = (2.0 * g) / fbn
  k_vel = (2.0 * (w[0] * g)) / fbn
  k = np.where(np.arange(d) < dof, k_pos, k_vel)
  gu = m * k
  store = (lambda a: np.asarray(a, np.float64)) if io == 'f64' else (lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64))
  ge, go = c_ext / fb, (w[1] * c_ext) / fb
  return dict(update=store(gu), target=store(-gu), target_sub=store(gu), sg=store(np.full(B, ge)), gp=store(np.full(B, ge)), obs=store(np.full(B, go)))


def sum_bound(n_addends):
  """relative bound of a sum of n_addends non-negative addends against the same sum in another order, with the divisions and weighted combinations behind it"""
  return (n_addends + 8) * U
