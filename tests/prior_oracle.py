"""numpy fp64 restatement of dgp_prior_samples (include/dgpmp2_hip.h), written independently of the kernel: its own Philox4x32-10 and Box-Muller normals, the host
constants (Cholesky, SPD inverse, S) in plain Python floats in the header's order, the two prefix scans in the header's association order and Matheron's rule.
Python floats and numpy's element-wise + - * / are IEEE binary64 and neither contracts a * b + c, so with SUPPLIED noise this file and the kernel agree bit for bit
(tests/test_hip_prior.py); the generated normals go through this platform's log / cos / sin and agree to 1e-13.  tests/test_prior_oracle.py holds this file against
the definition: the dense (A^T K^-1 A)^-1 and its solve."""
import math

import numpy as np

STREAM_TAG = 0x50
MAX_SAMPLES = 1 << 24
M32 = np.uint64(0xffffffff)
TWO_PI = 6.283185307179586


def lpt(n):
  """lanes per trajectory the kernel runs n states with; past 64 states: the block loop (is_long)"""
  return 16 if n <= 16 else (32 if n <= 32 else 64)


def is_long(n): return n > 64


# ---- randomness ----------------------------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
  """Philox4x32, 10 rounds, on uint64 arrays holding 32-bit words -> four arrays of words"""
  c0, c1, c2, c3 = [np.asarray(v, dtype=np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
  k0, k1 = np.uint64(int(k0) & 0xffffffff), np.uint64(int(k1) & 0xffffffff)
  for r in range(10):
    if r: k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
  return c0, c1, c2, c3


def counters(problem, s, n, d):
  """the (n + 1) d / 2 counters (4-tuples of ints) of trajectory (problem, s)"""
  return [(problem & 0xffffffff, (problem >> 32) & 0xffffffff, j, (STREAM_TAG << 24) | s) for j in range((n + 1) * d // 2)]


def normals(seed, problem, s, n, d):
  """the (n + 1, d) standard normals of trajectory (problem, s) under `seed`"""
  nb = (n + 1) * d // 2
  j = np.arange(nb, dtype=np.uint64)
  w = philox4x32_10(np.uint64(problem & 0xffffffff), np.uint64((problem >> 32) & 0xffffffff), j, np.uint64((STREAM_TAG << 24) | s), seed & 0xffffffff, (seed >> 32) & 0xffffffff)
  u0 = (((w[0] << np.uint64(32)) | w[1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
  u1 = (((w[2] << np.uint64(32)) | w[3]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
  r = np.sqrt(-2.0 * np.log(1.0 - u0))
  a = TWO_PI * u1
  return np.stack([r * np.cos(a), r * np.sin(a)], axis=1).reshape(n + 1, d)


def all_normals(seed, first_problem, B, S, n, d):
  return np.stack([np.stack([normals(seed, first_problem + b, s, n, d) for s in range(S)]) for b in range(B)])


# ---- host constants, plain Python floats ---------------------------------------------------------------------------------------------------------------------------
def cholesky(A):
  """lower factor of the symmetric matrix A (list of rows; the lower triangle is read) or None where a pivot is not positive and finite"""
  N = len(A)
  G = [[0.0] * N for _ in range(N)]
  for j in range(N):
    s = A[j][j]
    for k in range(j): s = s - G[j][k] * G[j][k]
    if not (s > 0.0) or not (s < math.inf): return None
    G[j][j] = math.sqrt(s)
    for i in range(j + 1, N):
      r = A[i][j]
      for k in range(j): r = r - G[i][k] * G[j][k]
      G[i][j] = r / G[j][j]
  return G


def spd_inverse(A):
  N = len(A)
  G = cholesky(A)
  if G is None: return None
  V = [[0.0] * N for _ in range(N)]
  for j in range(N):
    V[j][j] = 1.0 / G[j][j]
    for i in range(j + 1, N):
      s = G[i][j] * V[j][j]
      for k in range(j + 1, i): s = s + G[i][k] * V[k][j]
      V[i][j] = (-s) / G[i][i]
  out = [[0.0] * N for _ in range(N)]
  for i in range(N):
    for j in range(i + 1):
      s = V[i][i] * V[i][j]
      for k in range(i + 1, N): s = s + V[k][i] * V[k][j]
      out[i][j] = out[j][i] = s
  return out


def p_coef(ks2, t):
  """coefficients of P(t) = K_s^2 Phi Phi^T + Q(t) (t: a float or an array): i_pp, i_pv, q_pp, q_pv, q_vv"""
  t2 = t * t
  t3 = t2 * t
  return ks2 * (1.0 + t2), ks2 * t, t3 / 3.0, t2 / 2.0, t


class Consts(object):
  """what dgp_prior.h forms on the host from a handle's configuration (p: oracle.gpmp2_oracle.OracleParams or anything with its fields)"""

  def __init__(self, p):
    dof, n = int(p.dof), int(p.n)
    A = [[float(v) for v in row] for row in np.asarray(p.Q_c_inv, dtype=np.float64)]
    if any(A[i][j] != A[j][i] for i in range(dof) for j in range(i)): raise ValueError('Q_c_inv is not symmetric')
    self.Qc = spd_inverse(A)
    self.Lc = cholesky(self.Qc) if self.Qc is not None else None
    if self.Lc is None: raise ValueError('Q_c_inv is not symmetric positive definite')
    self.dof, self.d, self.n = dof, 2 * dof, n
    self.dt = float(p.total_time_sec) * 1.0 / float(n - 1) * 1.0
    self.t_end = float(n - 1) * self.dt
    self.ks, self.kg = float(p.K_s), float(p.K_g)
    self.ks2 = self.ks * self.ks
    kg2 = self.kg * self.kg
    sdt, s3 = math.sqrt(self.dt), math.sqrt(3.0)
    self.cp, self.cv1, self.cv2 = (self.dt * sdt) / s3, (s3 / 2.0) * sdt, sdt / 2.0
    i_pp, i_pv, q_pp, q_pv, q_vv = p_coef(self.ks2, self.t_end)
    d = self.d
    Sm = [[0.0] * d for _ in range(d)]
    for i in range(dof):
      for j in range(dof):
        q, e = self.Qc[i][j], 1.0 if i == j else 0.0
        Sm[i][j] = (i_pp + kg2) * e + q_pp * q
        Sm[i][dof + j] = Sm[dof + i][j] = i_pv * e + q_pv * q
        Sm[dof + i][dof + j] = (self.ks2 + kg2) * e + q_vv * q
    self.Sinv = spd_inverse(Sm)
    if self.Sinv is None: raise ValueError('S is not positive definite')
    self.x_lims, self.y_lims = tuple(p.x_lims), tuple(p.y_lims)


# ---- the construction, vectorised over leading axes ------------------------------------------------------------------------------------------------------------------
def mat_vec(M, x, lower=False):
  """(M x) with every row summed left to right; x (..., N) -> (..., N); lower: over j <= i only"""
  N = len(M)
  out = []
  for i in range(N):
    s = M[i][0] * x[..., 0]
    for j in range(1, (i + 1) if lower else N): s = s + M[i][j] * x[..., j]
    out.append(s)
  return np.stack(out, axis=-1)


def scan(e):
  """the header's SCAN along the last axis"""
  e = np.array(e, dtype=np.float64)
  n = e.shape[-1]
  for k0 in range(0, n, 64):
    blk = e[..., k0:k0 + 64]
    off = 1
    while off < 64:
      if off < blk.shape[-1]:
        new = blk.copy()
        new[..., off:] = blk[..., :-off] + blk[..., off:]
        blk[...] = new
      off *= 2
    if k0 > 0: blk[...] = e[..., k0 - 1:k0] + blk
  return e


def apply_w(k, t, g):
  """W(t_k) g for every state: t (n,), g (..., d) -> (..., n, d)"""
  dof = k.dof
  tau = k.t_end - t
  i_pp, i_pv, q_pp, q_pv, q_vv = p_coef(k.ks2, t)
  g = g[..., None, :]
  hv = tau[:, None] * g[..., :dof] + g[..., dof:]
  hp = np.broadcast_to(g[..., :dof], hv.shape)
  ap = q_pp[:, None] * hp + q_pv[:, None] * hv
  av = q_pv[:, None] * hp + q_vv[:, None] * hv
  qp, qv = mat_vec(k.Qc, ap), mat_vec(k.Qc, av)
  return np.concatenate([(i_pp[:, None] * hp + i_pv[:, None] * hv) + qp, (i_pv[:, None] * hp + k.ks2 * hv) + qv], axis=-1)


def chain(k, z):
  """the unconditioned chain: z (..., n + 1, d) -> x (..., n, d)"""
  dof, n = k.dof, k.n
  rows = z[..., :n, :]
  lu, lw = mat_vec(k.Lc, rows[..., :dof], lower=True), mat_vec(k.Lc, rows[..., dof:], lower=True)
  ev = k.cv1 * lu + k.cv2 * lw
  ev[..., 0, :] = k.ks * z[..., 0, dof:]
  v = np.moveaxis(scan(np.moveaxis(ev, -2, -1)), -1, -2)
  ep = k.cp * lu
  ep[..., 1:, :] = ep[..., 1:, :] + k.dt * v[..., :-1, :]
  ep[..., 0, :] = k.ks * z[..., 0, :dof]
  p = np.moveaxis(scan(np.moveaxis(ep, -2, -1)), -1, -2)
  return np.concatenate([p, v], axis=-1)


def rnd(a, io): return np.asarray(a, dtype=np.float32).astype(np.float64) if io == 'f32' else np.asarray(a, dtype=np.float64)


def run(p, start, goal, noise, mean=None, scale=1.0, io='f64'):
  """start, goal (B,1,d), noise (B,S,n+1,d), mean (B,n,d) or None -> th (B,S,n,d) as float64 holding io-rounded values, info (B,S) int32.
  The inputs are taken as they are: round them to io first (rnd)."""
  with np.errstate(invalid='ignore', over='ignore'):      # (non-finite noise is a test input: it must come out as info bit 1, not as a warning)
    return _run(p, start, goal, noise, mean, scale, io)


def _run(p, start, goal, noise, mean, scale, io):
  k = Consts(p)
  dof, n = k.dof, k.n
  start, goal, z = np.asarray(start, dtype=np.float64)[:, 0], np.asarray(goal, dtype=np.float64)[:, 0], np.asarray(noise, dtype=np.float64)
  t = np.arange(n).astype(np.float64) * k.dt
  x = chain(k, z)
  y = x[..., n - 1, :] + k.kg * z[..., n, :]
  wy = apply_w(k, t, mat_vec(k.Sinv, y))
  if mean is not None: m = np.asarray(mean, dtype=np.float64)[:, None]
  else:
    sp, sv = start[:, :dof], start[:, dof:]
    r0 = np.concatenate([goal[:, :dof] - (sp + k.t_end * sv), goal[:, dof:] - sv], axis=-1)
    wr = apply_w(k, t, mat_vec(k.Sinv, r0))
    m = np.concatenate([(sp[:, None] + t[:, None] * sv[:, None]) + wr[..., :dof], sv[:, None] + wr[..., dof:]], axis=-1)[:, None]
  th = rnd(m + float(scale) * (x - wy), io)
  out = ~((th[..., 0] >= k.x_lims[0]) & (th[..., 0] <= k.x_lims[1]) & (th[..., 1] >= k.y_lims[0]) & (th[..., 1] <= k.y_lims[1]))
  info = out.any(-1).astype(np.int32) | (2 * (~np.isfinite(th)).any((-1, -2)).astype(np.int32))
  return th, info


def mu(p, start, goal, io='f64'):
  """the prior mean (B,n,d): run at scale 0 without a mean (the noise is multiplied by zero)"""
  k = Consts(p)
  B = np.asarray(start).shape[0]
  return run(p, start, goal, np.zeros((B, 1, k.n + 1, k.d)), None, 0.0, io)[0][:, 0]


def linear_map(p):
  """M ((n d), (n + 1) d): column i is xi for the i-th unit noise -- Cov(xi) = M M^T"""
  k = Consts(p)
  N = (k.n + 1) * k.d
  z = np.eye(N).reshape(1, N, k.n + 1, k.d)
  zero = np.zeros((1, 1, k.d))
  th, _ = run(p, zero, zero, z, mean=np.zeros((1, k.n, k.d)), scale=1.0)
  return th[0].reshape(N, k.n * k.d).T
