"""Inputs shared by tests/test_loss_oracle.py (CPU) and tests/test_hip_loss.py (GPU): batches for dgp_step_loss in which, side by side in every wavefront, some
trajectories have an update equal to the expert's (a miss of exactly 0), some are large, some have zero errors and the rest are ordinary.  Every value is a small
multiple of 2^-10: exactly representable in fp32, and target - target_sub is exact in either type, so the fp32 and fp64 runs see the same numbers."""
import numpy as np

WEIGHTS = ((0.5, 2.0, 0.3), (0.0, 1.0, 1.0))      # (vel_loss_lambda, ext_obs_lambda, ext_loss_weight): the fixture's two sets


def bits(a):
  a = np.ascontiguousarray(a, dtype=np.float64)
  return a.view(np.uint64)


def same_bits(a, b):
  """bit for bit, any NaN equal to any NaN"""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _grid(rs, shape, scale=1.0):
  return rs.randint(-4096, 4097, shape).astype(np.float64) / 1024.0 * scale


def mixed_batch(dof, n, B, seed=0):
  """-> dict(update, target, target_sub (B,n,d); sg, gp, obs (B), non-negative).  Trajectory b by b % 4: 0 the update is the expert's (update == target - target_sub
  exactly), 1 large (entries up to 4096), 2 zero errors, 3 ordinary."""
  rs = np.random.RandomState(1000 * dof + 7 * n + 31 * B + seed)
  d = 2 * dof
  upd, tgt, sub = _grid(rs, (B, n, d)), _grid(rs, (B, n, d)), _grid(rs, (B, n, d))
  kind = np.arange(B) % 4
  big = kind == 1
  upd[big] *= 1024.0; tgt[big] *= 1024.0; sub[big] *= 1024.0
  hit = kind == 0
  upd[hit] = tgt[hit] - sub[hit]
  sg, gp, obs = (rs.randint(0, 4097, B).astype(np.float64) / 256.0 for _ in range(3))
  none = kind == 2
  sg[none] = 0.0; gp[none] = 0.0; obs[none] = 0.0
  return dict(update=upd, target=tgt, target_sub=sub, sg=sg, gp=gp, obs=obs)
