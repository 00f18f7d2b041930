"""Inputs shared by tests/test_prior_oracle.py (CPU) and tests/test_hip_prior.py (GPU): configurations, seeded problems and the motivating multi-start scene."""
import numpy as np

import prior_oracle as PO
from oracle import gpmp2_oracle as O

# non-diagonal SPD Q_c_inv (fp32-exact entries)
QC_FULL = {2: np.array([[2.0, 0.5], [0.5, 1.25]]), 3: np.array([[2.0, 0.5, 0.25], [0.5, 1.25, -0.375], [0.25, -0.375, 1.5]])}
QC_DIAG = {2: np.diag([1.0, 1.0]), 3: np.diag([1.0, 1.0, 1.0])}


def params(dof, n, qc='diag', **kw):
  """qc: 'diag' (identity: the reference's configuration), 'full' (QC_FULL) or a matrix"""
  Q = QC_DIAG[dof] if isinstance(qc, str) and qc == 'diag' else (QC_FULL[dof] if isinstance(qc, str) else np.asarray(qc, dtype=np.float64))
  return O.OracleParams(dof=dof, total_time_step=n - 1, Q_c_inv=Q, **kw)


def inputs(dof, n, B, S, seed, io='f64', with_mean=True):
  """-> start, goal (B,1,d), mean (B,n,d) or None, noise (B,S,n+1,d): seeded, start / goal / mean rounded to io (what the kernel reads), the noise doubles"""
  rs = np.random.RandomState(seed)
  d = 2 * dof
  start = np.concatenate([rs.uniform(-4, 4, (B, 1, dof)), rs.uniform(-0.5, 0.5, (B, 1, dof))], -1)
  goal = np.concatenate([rs.uniform(-4, 4, (B, 1, dof)), rs.uniform(-0.5, 0.5, (B, 1, dof))], -1)
  mean = rs.uniform(-3, 3, (B, n, d)) if with_mean else None
  noise = rs.randn(B, S, n + 1, d)
  return PO.rnd(start, io), PO.rnd(goal, io), (None if mean is None else PO.rnd(mean, io)), noise


def bits(a):
  a = np.ascontiguousarray(a, dtype=np.float64)
  return a.view(np.uint64)


def same_bits(a, b):
  """equal as bit patterns, every NaN equal to every NaN"""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the motivating case: one disc on the segment from the start to the goal ------------------------------------------------------------------------------------------
# Gauss-Newton from the straight line stays in collision (the line runs through the disc's centre, where the lateral gradient of the hinge cost all but vanishes);
# among MOTIV_S samples of the prior at MOTIV_SCALE -- mid-trajectory standard deviation sqrt(T^3 / 192) = 2.3, the disc's diameter -- several end collision-free.
# Confirmed on the CPU oracle's GN loop (oracle.planner_forward, 10 iterations, tol_delta 1e-4) with the oracle's own normals for MOTIV_SEED: the straight line
# ends with a dense maximum penetration of 0.039 and an error of 25.4; samples 3, 4, 5, 9, 11, 12, 14, 15 end collision-free (GP-interpolated check, 7 states per
# interval) with errors of 0.006 .. 0.021; samples 0 and 9 leave the limits on the way (info bit 0).
MOTIV_N, MOTIV_G, MOTIV_S, MOTIV_SEED, MOTIV_SCALE, MOTIV_ITERS, MOTIV_INTER = 17, 64, 16, 0, 1.0, 10, 7
MOTIV_FREE = (3, 4, 5, 9, 11, 12, 14, 15)


def motivating_case():
  """-> p, start (1,1,4), goal (1,1,4), straight line (1,n,4), sdf (1,1,G,G)"""
  p = params(2, MOTIV_N)
  sdf = O.circles_sdf(MOTIV_G, ((0.0, 0.0, 1.0),))[None, None]
  start, goal = np.array([[[-3.5, 0.0, 0.0, 0.0]]]), np.array([[[3.5, 0.0, 0.0, 0.0]]])
  line = O.straight_line_trajb(start[:, :, :2], goal[:, :, :2], p.total_time_sec, MOTIV_N - 1, 2)
  return p, start, goal, line, sdf
