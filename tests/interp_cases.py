"""Inputs shared by tests/test_interp_oracle.py (CPU) and tests/test_hip_interp.py (GPU): the motivating case of dgp_gp_interpolate -- a trajectory whose support
states clear an obstacle that the path between them crosses -- and small lane-mixed batches for every shape of the GPU file."""
import numpy as np

import parity_cases as PC
from oracle import gpmp2_oracle as O

DISC = ((-1.25, 0.0, 0.3),)       # one small disc: with the robot's radius 0.4 a state collides within ~0.7 of its centre
CIRCLES = ((-2.0, -1.0, 1.0), (1.5, 2.0, 0.8), (0.0, 0.0, 0.7))


def disc_sdf(G=16):
  """(1, 1, G, G): circles_sdf of DISC, fp32-exact numbers"""
  return PC.rnd(O.circles_sdf(G, DISC)[None, None], 'f32')


def motivating_case(G=16):
  """-> (p, th (1,3,4), sdf (1,1,G,G)): a 3-state constant-velocity straight line along y = 0 from x = -2.5 to x = 2.5 over 10 s; its states (x = -2.5, 0, 2.5) are
  at least 0.9 from the disc's rim, its first interval passes through the disc's centre"""
  p = O.OracleParams(dof=2, total_time_sec=10.0, total_time_step=2)
  start, goal = np.array([[[-2.5, 0.0]]]), np.array([[[2.5, 0.0]]])
  return p, O.straight_line_trajb(start, goal, 10.0, 2, 2), disc_sdf(G)


def grid(hw):
  """(1, 1, H, W) from circles_sdf of CIRCLES, cropped to hw (res = 10 / W), fp32-exact numbers"""
  return PC.rnd(O.circles_sdf(max(hw), CIRCLES)[None, None, :hw[0], :hw[1]], 'f32')


def mixed_batch(dof, n, B, hw, seed=0):
  """-> (p, th (B,n,d), sdf (1,1,H,W)): straight lines with noise (positions and velocities), fp32-exact; trajectory b is of kind b % 4 -- 0: through the circles
  (colliding), 1: in the free corridor at the top, 2: leaving the grid through x = 5, 3: outside the grid entirely -- so every wavefront of every lanes-per-
  trajectory count holds colliding, free and out-of-grid trajectories side by side"""
  rs = np.random.RandomState(seed)
  d = 2 * dof
  p = O.OracleParams(dof=dof, total_time_step=n - 1, non_holonomic=dof == 3)
  kind = np.arange(B) % 4
  start, goal = np.zeros((B, 1, dof)), np.zeros((B, 1, dof))
  start[:, 0, :2], goal[:, 0, :2] = rs.uniform(-4, 4, (B, 2)), rs.uniform(-4, 4, (B, 2))
  k = kind == 0
  start[k, 0, :2], goal[k, 0, :2] = rs.uniform(-3.0, -1.0, (k.sum(), 2)), rs.uniform(0.5, 2.5, (k.sum(), 2))
  k = kind == 1
  start[k, 0, 0], goal[k, 0, 0] = rs.uniform(-4.4, -3.0, k.sum()), rs.uniform(3.0, 4.4, k.sum())
  start[k, 0, 1], goal[k, 0, 1] = rs.uniform(4.2, 4.4, k.sum()), rs.uniform(4.2, 4.4, k.sum())
  k = kind == 2
  goal[k, 0, 0] = rs.uniform(6.0, 8.0, k.sum())
  k = kind == 3
  start[k, 0, 0], goal[k, 0, 0] = rs.uniform(5.5, 8.0, k.sum()), rs.uniform(5.5, 8.0, k.sum())
  if dof == 3: goal[:, 0, 2] = rs.uniform(-np.pi, np.pi, B)
  th = O.straight_line_trajb(start, goal, 10.0, n - 1, dof) + rs.randn(B, n, d) * np.where(kind == 1, 0.005, 0.05)[:, None, None]
  return p, PC.rnd(th, 'f32'), grid(hw)


def bits(a):
  """the bit patterns of a float64 array (NaN and -0.0 compare by their bits)"""
  return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_bits(a, b):
  """float arrays equal bit for bit, any NaN equal to any NaN (a float32 NaN widened on the way keeps no particular payload)"""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
