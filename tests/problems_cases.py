"""Inputs of the problem-sampler tests (tests/test_hip_problems.py, tests/test_problems_oracle.py): small synthetic signed distance fields that force every branch of
dgp_sample_problems, mixed inside every wavefront, and the oracle's answer for them (tests/problems_oracle.py), computed once per input and shared.

Fields over [-5, 5]^2, values -1 (obstacle) and +3 (free) only: fp32 numbers, so fp32 and fp64 I/O read the same grid.  With the clearance of 0.9:
  EMPTY    free everywhere (but the last row / column, where the reference's clamped taps cancel): most first draws are accepted
  CLUTTER  two pockets of 2 x 2 free cells in opposite corners: ~2 % of the box is feasible, the accepted draw index usually exceeds the 16 lanes of a problem
  BLOCKED  no feasible point: both loops hit max_draws
  POCKET   one pocket of free cells narrower than the distance wanted of a goal: no far goal exists, the 17th feasible-but-near candidate is accepted (bit 2)
  CORNERS  free, but for obstacles on the two lower corners: every one of the four diagonals has an infeasible end and falls back to a random problem (bit 3)
Problem b of a batch: environment KINDS[b % 5], so the four problems of a wavefront's lane groups differ; diagonal (b // 5) % 5 - 1 (-1: random), so the EMPTY and the
CORNERS problems see every diagonal.  corner_inset = 1.0: on grids this coarse the reference's own 0.2 puts every corner into the last row / column."""
import functools

import numpy as np

import problems_oracle as PO

EMPTY, CLUTTER, BLOCKED, POCKET, CORNERS = range(5)
CLEARANCE, MAX_DRAWS, INSET, T_SEC = 0.9, 256, 1.0, 10.0
SIZES = {3: (16, 16), 16: (22, 18), 101: (32, 32)}      # num_states -> (H, W): a multiple of the 4 x 4 tile, a non-square one that is not, the largest
B_MAIN = 64 * 2 + 3                                      # two wavefronts' worth of lanes even at one problem per lane, and a ragged tail


def fields(H, W):
  """(5, H, W) float64"""
  f = np.full((5, H, W), -1.0)
  S = W                     # rows 0 .. W - 1 lie inside the (square) limits whatever H is: res = 10 / W
  f[EMPTY] = 3.0
  f[CLUTTER, 2:5, 2:5] = 3.0
  f[CLUTTER, S - 5:S - 2, S - 5:S - 2] = 3.0
  h = S // 5
  f[POCKET, S // 2 - h:S // 2 + h + 1, S // 2 - h:S // 2 + h + 1] = 3.0      # 2 h res < 0.6 x the box diagonal
  f[CORNERS] = 3.0
  f[CORNERS, S - S // 4 - 1:, :S // 4] = -1.0
  f[CORNERS, S - S // 4 - 1:, S - S // 4:] = -1.0
  return f


def params():
  return PO.Params(CLEARANCE, max_draws=MAX_DRAWS, corner_inset=INSET, total_time_sec=T_SEC)


def layout(B):
  b = np.arange(B)
  return (b % 5).astype(np.int32), ((b // 5) % 5 - 1).astype(np.int32)      # env_index, diagonal


@functools.lru_cache(maxsize=None)
def mixed(H, W, B=B_MAIN, seed=7, first_problem=0):
  """-> (fields, env_index, diagonal, (start, goal, draws, info)) -- read-only, shared between tests"""
  f = fields(H, W)
  env, diag = layout(B)
  if first_problem: env, diag = layout(first_problem + B)[0][first_problem:], layout(first_problem + B)[1][first_problem:]
  out = PO.sample_problems(f, params(), B, seed, first_problem, env, diag)
  for a in (f, env, diag) + out: a.setflags(write=False)
  return f, env, diag, out


@functools.lru_cache(maxsize=None)
def shared(H, W, B=B_MAIN, seed=11):
  """one grid (CORNERS) for the whole batch, diagonals mixed"""
  f = fields(H, W)[CORNERS:CORNERS + 1]
  _, diag = layout(B)
  out = PO.sample_problems(f, params(), B, seed, 0, None, diag)
  for a in (f, diag) + out: a.setflags(write=False)
  return f, None, diag, out


def branch_counts(env, diag, draws, info):
  """how often each branch the issue lists occurs"""
  rnd = (diag < 0) | ((info & 8) != 0)
  return {'first_draw': int(np.sum((env == EMPTY) & rnd & (draws[:, 0] == 0))),      # (the start loop's: a first goal draw must also land far enough away)
          'beyond_group': int(np.sum((env == CLUTTER) & ((draws[:, 0] >= 16) | (draws[:, 1] >= 16)) & ((info & 3) == 0))),
          'both_caps': int(np.sum((env == BLOCKED) & ((info & 3) == 3))),
          'near_tries': int(np.sum((env == POCKET) & ((info & 4) != 0))),
          'diagonal_kept': [int(np.sum((env == EMPTY) & (diag == d) & (info == 0) & (draws[:, 0] == -1))) for d in range(4)],
          'diagonal_replaced': [int(np.sum((env == CORNERS) & (diag == d) & ((info & 8) != 0))) for d in range(4)]}


def check_branches(c):
  assert c['first_draw'] > 0 and c['beyond_group'] > 0 and c['both_caps'] > 0 and c['near_tries'] > 0, c
  assert min(c['diagonal_kept']) > 0 and min(c['diagonal_replaced']) > 0, c


# ---- away from the default limits and horizon: x and y limits that differ from each other and are not symmetric, total_time_sec = 7 ------------------------------
# res = 10 / 20 = 0.5; rows follow py = -y_lims[0] / res - y / res = 12 - 2 y (env_2d.py:60-62), so the box y in [-6, 2] lies in rows 8 ... 24 of 26 and rows 0 ... 7 are
# never read (y > 2 is outside the limits); columns 0 ... 20 hold x in [-3, 7].  The fields keep the kinds and the branch each one forces.
ND_X, ND_Y, ND_T_SEC, ND_HW, ND_N = (-3.0, 7.0), (-6.0, 2.0), 7.0, (26, 20), 16


def fields_nd():
  """(5, 26, 20) float64"""
  f = np.full((5,) + ND_HW, -1.0)
  f[EMPTY] = 3.0
  f[CLUTTER, 10:13, 2:5] = 3.0
  f[CLUTTER, 20:23, 15:18] = 3.0
  f[POCKET, 14:19, 8:13] = 3.0
  f[CORNERS] = 3.0
  f[CORNERS, 19:, :5] = -1.0
  f[CORNERS, 19:, 15:] = -1.0
  return f


def params_nd(x_lims=ND_X, y_lims=ND_Y):
  return PO.Params(CLEARANCE, x_lims=x_lims, y_lims=y_lims, max_draws=MAX_DRAWS, corner_inset=INSET, total_time_sec=ND_T_SEC)


@functools.lru_cache(maxsize=None)
def mixed_nd(B=B_MAIN, seed=7, x_lims=ND_X, y_lims=ND_Y):
  """mixed() on fields_nd() at the limits given (default: ND_X, ND_Y)"""
  f = fields_nd()
  env, diag = layout(B)
  out = PO.sample_problems(f, params_nd(x_lims, y_lims), B, seed, 0, env, diag)
  for a in (f, env, diag) + out: a.setflags(write=False)
  return f, env, diag, out


@functools.lru_cache(maxsize=None)
def shared_nd(B=B_MAIN, seed=11):
  f = fields_nd()[CORNERS:CORNERS + 1]
  _, diag = layout(B)
  out = PO.sample_problems(f, params_nd(), B, seed, 0, None, diag)
  for a in (f, diag) + out: a.setflags(write=False)
  return f, None, diag, out
