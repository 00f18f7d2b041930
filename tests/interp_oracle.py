"""numpy fp64 restatement of dgp_gp_interpolate (include/dgpmp2_hip.h: the GP-interpolated dense trajectory, the hinge cost of every dense state and the DGP_DENSE_*
summary), in the header's operation order -- numpy's elementwise ufuncs do not contract a multiply and an add, so dense() gives the kernel's bits -- and the same rule
built from its definition: Lambda, Psi from Phi, Q_tau, Q_Delta^-1 (gp/gp_factor.py:31-53) as matrices in np.longdouble for a given SPD Q_c.  The lookup is that of
tests/metrics_oracle.obs_error (oracle.gpmp2_oracle's bilinear lookup / hinge)."""
import numpy as np

import metrics_oracle as MO

NAMES = ('in_coll', 'num_colliding', 'avg_penetration', 'max_penetration', 'first_colliding', 'worst_index')
COL = {k: i for i, k in enumerate(NAMES)}
EXACT = [COL[k] for k in ('in_coll', 'num_colliding', 'first_colliding', 'worst_index')]


def num_dense(n, K): return (n - 1) * (K + 1) + 1


def lpt(nd):
  """lanes per trajectory of the kernel for nd dense states: mirror of dgp_host::dense_lpt (csrc/dgp_host.h), for asserting which instantiations a test reaches"""
  return 16 if nd <= 64 else (32 if nd <= 128 else 64)


def times(p, K):
  """(N_d,): i dt + j dt / (K + 1)"""
  m = np.arange(num_dense(p.n, K))
  return (m // (K + 1)) * p.dt + (m % (K + 1)) * p.dt / (K + 1)


def coefficients(s, dt):
  """the eight coefficients at offsets s (array), in the header's operation order -> a0, a1, a2, a3, b0, b1, b2, b3"""
  s2 = s * s
  s3 = s2 * s
  a0 = (1.0 - 3.0 * s2) + 2.0 * s3
  a1 = dt * ((s - 2.0 * s2) + s3)
  a2 = 3.0 * s2 - 2.0 * s3
  a3 = dt * (s3 - s2)
  b2 = (6.0 * (s - s2)) / dt
  b0 = -b2
  b1 = (1.0 - 4.0 * s) + 3.0 * s2
  b3 = 3.0 * s2 - 2.0 * s
  return a0, a1, a2, a3, b0, b1, b2, b3


def dense(p, th, K, dt=None):
  """(B, n, d) -> (B, N_d, d) float64: offset-0 rows are copies of the support rows (bit for bit), the others the closed form.  dt: p.dt unless given."""
  th = np.asarray(th, np.float64)
  B, n, d = th.shape
  dof, K1 = d // 2, K + 1
  dt = np.float64(p.dt if dt is None else dt)
  m = np.arange(num_dense(n, K))
  i, j = m // K1, m % K1
  i1 = np.minimum(i + 1, n - 1)
  s = j.astype(np.float64) / np.float64(K1)
  c = [v[None, :, None] for v in coefficients(s, dt)]
  x0, v0, x1, v1 = th[:, i, :dof], th[:, i, dof:], th[:, i1, :dof], th[:, i1, dof:]
  out = np.empty((B, len(m), d))
  with np.errstate(invalid='ignore'):
    out[:, :, :dof] = ((c[0] * x0 + c[1] * v0) + c[2] * x1) + c[3] * v1
    out[:, :, dof:] = ((c[4] * x0 + c[5] * v0) + c[6] * x1) + c[7] * v1
  cp = j == 0
  out[:, cp] = th[:, i[cp]]
  return out


def cost(p, th_dense, sdf, eps):
  """(B, N_d): raw hinge cost of every dense state at epsilon `eps`; sdf (B | 1, 1, H, W)"""
  with np.errstate(invalid='ignore'):
    return MO.obs_error(p, th_dense, sdf, eps)


def summary(c):
  """dense costs (B, N_d) float64 -> (B, 6) float64 in the order of NAMES, over the dense states 1 .. N_d - 2 (the mean summed in state order)"""
  c = np.asarray(c, np.float64)
  B, nd = c.shape
  assert nd >= 3
  inner = c[:, 1:-1]
  S = np.zeros((B, len(NAMES)))
  hit = inner != 0.0                                   # a NaN counts
  cnt = hit.sum(1)
  S[:, COL['num_colliding']] = cnt
  S[:, COL['in_coll']] = cnt > 0
  acc = np.zeros(B)
  for k in range(nd - 2): acc = acc + inner[:, k]
  S[:, COL['avg_penetration']] = acc / float(nd - 2)
  nan = np.isnan(inner)
  with np.errstate(invalid='ignore'):
    S[:, COL['max_penetration']] = np.max(inner, axis=1)      # a NaN wins
  S[:, COL['first_colliding']] = np.where(cnt > 0, np.argmax(hit, axis=1) + 1, -1)
  S[:, COL['worst_index']] = np.where(nan.any(1), np.argmax(nan, axis=1), np.argmax(np.where(nan, -np.inf, inner), axis=1)) + 1      # the first NaN, else the first maximum
  return S


def run(p, th, K, sdf=None, eps=0.0, io='f64'):
  """what the kernel must give for inputs th / sdf (numbers exact in `io`): th_dense, dense_cost (both as float64 holding io-rounded values) and the summary.
  fp32: the interpolation and the lookup in fp64 at the unrounded positions, every stored value rounded once."""
  rnd = (lambda a: a) if io == 'f64' else (lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64))
  d64 = dense(p, th, K)
  if sdf is None: return rnd(d64), None, None
  c64 = cost(p, d64, sdf, eps)
  return rnd(d64), rnd(c64), (summary(c64) if d64.shape[1] >= 3 else None)


def _inv_ld(A):
  """Gauss-Jordan inverse with partial pivoting in np.longdouble (numpy.linalg has no extended precision)"""
  A = np.array(A, np.longdouble)
  k = A.shape[0]
  M = np.concatenate([A, np.eye(k, dtype=np.longdouble)], axis=1)
  for c in range(k):
    piv = c + int(np.argmax(np.abs(M[c:, c])))
    M[[c, piv]] = M[[piv, c]]
    M[c] = M[c] / M[c, c]
    for r in range(k):
      if r != c: M[r] = M[r] - M[r, c] * M[c]
  return M[:, k:]


def lambda_psi(dof, dt, tau, Qc):
  """Lambda(tau), Psi(tau) (d x d, np.longdouble) from the definition: Psi = Q_tau Phi(dt - tau)^T Q_dt^-1, Lambda = Phi(tau) - Psi Phi(dt); Phi, Q, Q^-1 as
  gp/gp_factor.py:31-53 builds them (Q^-1 from Q_c^-1 with the factors 12 dt^-3, -6 dt^-2, 4 dt^-1)"""
  L = np.longdouble
  I, Z = np.eye(dof, dtype=L), np.zeros((dof, dof), L)
  Qc = np.array(Qc, L)
  Qci = _inv_ld(Qc)
  dt, tau = L(dt), L(tau)
  phi = lambda t: np.block([[I, t * I], [Z, I]])
  Q = lambda t: np.block([[t ** 3 / L(3) * Qc, t ** 2 / L(2) * Qc], [t ** 2 / L(2) * Qc, t * Qc]])
  Qinv = np.block([[L(12) / dt ** 3 * Qci, L(-6) / dt ** 2 * Qci], [L(-6) / dt ** 2 * Qci, L(4) / dt * Qci]])
  psi = Q(tau) @ phi(dt - tau).T @ Qinv
  lam = phi(tau) - psi @ phi(dt)
  return lam, psi


def dense_from_definition(p, th, K, Qc, dt=None):
  """(B, N_d, d) np.longdouble: every dense state as Lambda(tau) theta_i + Psi(tau) theta_{i+1} with the matrices of lambda_psi (offset 0: tau = 0, Lambda = I, Psi = 0)"""
  L = np.longdouble
  th = np.asarray(th, np.float64).astype(L)
  B, n, d = th.shape
  dt = L(p.dt if dt is None else dt)
  K1 = K + 1
  out = np.empty((B, num_dense(n, K), d), L)
  mats = [lambda_psi(d // 2, dt, dt * L(j) / L(K1), Qc) for j in range(K1)]
  for m in range(out.shape[1]):
    i, j = divmod(m, K1)
    lam, psi = mats[j]
    out[:, m] = th[:, i] @ lam.T + th[:, min(i + 1, n - 1)] @ psi.T
  return out
