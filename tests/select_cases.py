"""Inputs shared by tests/test_select_oracle.py (CPU) and tests/test_hip_select.py (GPU): the base set -- tests/interp_cases.mixed_batch reshaped to (B,S) -- and the
additions that separate what the base set barely does (nearly every trajectory of it that leaves the limits also collides): trajectories whose END state alone is outside the
limits, exact score ties and a -0.0 / 0.0 pair inside tier 0 and inside tier 1, a NaN and a +inf score, a NaN stored velocity, `exclude` on the would-be winner."""
import numpy as np

import interp_cases as IC
import parity_cases as PC
from oracle import gpmp2_oracle as O

BS = ((1, 1), (5, 3), (7, 4), (3, 17), (2, 70))             # (problems, samples)
NK = ((3, 0), (17, 2), (65, 1), (33, 7))                     # (n, K): N_d = 3, 49, 129, 257
NK32 = (17, 4)                                               # N_d = 81: the 32-lane instantiation, which none of the four reaches
LPT = {(3, 0): 16, (17, 2): 16, (65, 1): 64, (33, 7): 64, NK32: 32}      # dgp_host::dense_lpt(N_d)
GRID = (16, 16)
F32_BELOW_M5 = float(np.nextafter(np.float32(-5.0), np.float32(-6.0)))      # the first float past x_min


def base(dof, n, B, S):
  """-> dict(p, th (B,S,n,d), sdf (1,1,16,16), score (B,S), exclude (B,S) zeros): mixed_batch(dof, n, B S, (16,16), seed=3), seeded fp32-exact positive scores"""
  p, th, sdf = IC.mixed_batch(dof, n, B * S, GRID, seed=3)
  score = PC.rnd(np.random.RandomState(100 + B * S).uniform(0.01, 30.0, (B, S)), 'f32')
  return dict(p=p, th=th.reshape(B, S, n, 2 * dof), sdf=sdf, score=score, exclude=np.zeros((B, S), np.int32))


def _line(dof, n, a, b):
  start, goal = np.zeros((1, 1, dof)), np.zeros((1, 1, dof))
  start[0, 0, :2], goal[0, 0, :2] = a, b
  if dof == 3: goal[0, 0, 2] = 0.5
  return PC.rnd(O.straight_line_trajb(start, goal, 10.0, n - 1, dof), 'f32')[0]


def additions(dof, n):
  """-> dict as base(): 3 problems x 8 samples on the same grid, hand-made.  `free`: straight lines in the free corridor at the top of the map; `coll_a` / `coll_b`:
  two lines through the circles; `end_out` / `start_out`: corridor lines whose last / first state alone lies one float past x_min (the lookup of the reference
  reads a distance of 0 in the last column and the last row of a grid, so a line that ends at x_max collides on the way there: both leave on the left).
    problem 0  s0 free 2.0 | s1 free 1.0 | s2 free 1.0 (tie: the index decides) | s3 free 0.0 | s4 free -0.0 (ties with s3) | s5 end_out -1.0 (wins only without
               require_inside) | s6 free with a NaN velocity, -5.0 | s7 free -3.0, excluded (the would-be winner).  Order 3 4 1 2 0 | 5 | 6 7.
    problem 1  no accepted sample: s0 coll_a 1.0 | s1 coll_a 1.0 (tie) | s2 coll_a 0.0 | s3 coll_a -0.0 (ties with s2) | s4 coll_b 5.0 | s5 start_out 0.5 (tier 1
               with penetration 0: ahead of every colliding sample) | s6 free, NaN score | s7 free, +inf score.
    problem 2  s0 coll_b 3.0 | s1 free 4.0 | s2 free 2.5 | s3 coll_a 0.1 | s4 free 7.0 | s5 coll_b 0.2, excluded | s6 end_out 9.0 | s7 free 2.5 (ties with s2)."""
  p = O.OracleParams(dof=dof, total_time_step=n - 1, non_holonomic=dof == 3)
  free = lambda k: _line(dof, n, (-4.0 + 0.125 * k, 4.25 + 0.03125 * k), (4.0 - 0.125 * k, 4.375 - 0.03125 * k))
  coll_a, coll_b = _line(dof, n, (-2.5, -1.5), (2.0, 2.25)), _line(dof, n, (-3.0, 0.25), (1.0, -0.25))
  end_out, start_out = _line(dof, n, (4.0, 4.3125), (F32_BELOW_M5, 4.3125)), _line(dof, n, (F32_BELOW_M5, 4.34375), (4.0, 4.34375))
  nan_vel = free(6).copy()
  nan_vel[n // 2, dof] = np.nan
  th = np.stack([np.stack([free(0), free(1), free(2), free(3), free(4), end_out, nan_vel, free(7)]),
                 np.stack([coll_a, coll_a, coll_a, coll_a, coll_b, start_out, free(1), free(2)]),
                 np.stack([coll_b, free(1), free(2), coll_a, free(4), coll_b, end_out, free(7)])])
  score = np.array([[2.0, 1.0, 1.0, 0.0, -0.0, -1.0, -5.0, -3.0],
                    [1.0, 1.0, 0.0, -0.0, 5.0, 0.5, np.nan, np.inf],
                    [3.0, 4.0, 2.5, 0.1, 7.0, 0.2, 9.0, 2.5]])
  exclude = np.zeros((3, 8), np.int32)
  exclude[0, 7], exclude[2, 5] = 1, 2
  return dict(p=p, th=th, sdf=IC.grid(GRID), score=PC.rnd(score, 'f32'), exclude=exclude)


def all_cases(dof, n):
  """the base set's five (B,S) and the additions"""
  return [('base B %d S %d' % bs, base(dof, n, *bs)) for bs in BS] + [('additions', additions(dof, n))]


def distinct_grids(sdf, B, seed=1):
  """one grid per PROBLEM: the shared one plus a constant each, fp32-exact (tests/test_hip_interp.per_sample's construction)"""
  return PC.rnd(sdf + np.random.RandomState(seed).uniform(-0.3, 0.3, (B, 1, 1, 1)), 'f32')


# ---- generate_dataset(multistart=...): two 32 x 32 environments, one diagonal problem each (corner_inset 1.0: from one corner (+-4, +-4) to the opposite one) -----------
# Environment 0 holds a disc of radius 2 on the centre of the map, which every diagonal crosses; environment 1 a small disc off both diagonals.  With DATASET_SEED
# generate_dataset draws diagonal 2 ((4,-4) -> (-4,4)) for environment 0 and diagonal 0 for environment 1.  Picked on the CPU oracle (oracle.planner_forward, n = 17,
# 10 iterations, tol_delta 1e-4, the GP-interpolated check with 7 states per interval; the samples from tests/prior_oracle.py's normals of (seed 3, problem e),
# mean = the straight line, scale 1.0): in environment 0 Gauss-Newton from the straight line stays in the disc (dense maximum penetration 0.81, error 180) and
# leaves the limits, all four samples end free and inside with errors 0.017, 0.035, 0.89, 0.017; in environment 1 the line and the four samples all end free (0.009).
# (On diagonals 0 and 1 the pixelated disc is not symmetric enough to hold the straight line: seeds 0 .. 2 draw those and Gauss-Newton escapes on its own.)
DATASET_SEED, DATASET_N, DATASET_S, DATASET_INTER = 3, 17, 4, 7


def dataset_images(S=32):
  c = -5.0 + (10.0 / S) * (np.arange(S) + 0.5)
  X, Y = np.meshgrid(c, c[::-1])
  im = np.ones((2, S, S))
  im[0][X ** 2 + Y ** 2 <= 2.0 ** 2] = 0.0
  im[1][(X - c[16]) ** 2 + (Y - 3.0) ** 2 <= 0.5 ** 2] = 0.0
  return im
