"""Plain numpy / Python fp64 restatement of dgp_shortcut_paths (include/dgpmp2_hip.h), scalar and literal, written independently of the kernel: the feasible point is
problems_oracle.signed_distance (the reference's Env2D.get_signed_obstacle_distance) above the clearance, a segment is visible where every point of the discrete
motion check is feasible, the greedy pass takes the farthest visible candidate, and the kept vertices go through
paths_oracle.resample.  Python floats are IEEE binary64 and Python never contracts a * b + c.
tests/test_shortcut_oracle.py holds this file against independent pins of the rule; tests/test_hip_shortcut.py holds the kernel against this file."""
import math

import numpy as np

import paths_oracle as PA
import problems_oracle as PO

BIT_NO_PATH, BIT_INPUT_TRUNCATED, BIT_VERTEX_TRUNCATED, BIT_UNVERIFIED = 1, 2, 4, 8
MAX_M = 2.0 ** 20


def vertices_of(cells, start, goal, W, x_lims, y_lims):
  """V_0 .. V_{L+1}: the start point itself, the points of the traced cells, the goal point itself"""
  return [(float(start[0]), float(start[1]))] + [PA.point_of(int(v) // W, int(v) % W, W, x_lims, y_lims) for v in cells] + [(float(goal[0]), float(goal[1]))]


def fmax(a, b):
  """C's fmax: the operand that is not a NaN"""
  if a != a: return b
  if b != b: return a
  return max(a, b)


def check_points(P, Q, check_step):
  """-> the M + 1 check points of the segment P Q, or None where m > 2^20"""
  dx, dy = Q[0] - P[0], Q[1] - P[1]
  m = fmax(abs(dx), abs(dy)) / check_step
  if m > MAX_M: return None
  M = 1 if not (m > 1) else int(math.ceil(m))
  return [(P[0] + (float(k) / float(M)) * dx, P[1] + (float(k) / float(M)) * dy) for k in range(M + 1)]


def visible(sdf, P, Q, clearance, check_step, x_lims, y_lims):
  """all M + 1 check points are feasible.  A pure predicate: the points are visited every 16th first, then every 4th, then the rest, so that a blocked segment
  is usually found out early -- the order decides nothing"""
  pts = check_points(P, Q, check_step)
  if pts is None: return False
  order = sorted(range(len(pts)), key=lambda k: (0 if k % 16 == 0 else 1 if k % 4 == 0 else 2, k))
  for k in order:
    if not PO.signed_distance(sdf, pts[k][0], pts[k][1], x_lims, y_lims) > clearance: return False
  return True


def greedy(sdf, V, clearance, check_step, lookahead, x_lims, y_lims):
  """-> (kept indices, unverified: a kept segment is not visible)"""
  last = len(V) - 1      # L + 1
  see = lambda i, j: visible(sdf, V[i], V[j], clearance, check_step, x_lims, y_lims)
  kept, a, unverified = [0], 0, False
  while a < last:
    hi = min(last, a + lookahead)
    best = next((j for j in range(hi, a + 1, -1) if see(a, j)), None)      # the largest visible j in [a + 2, hi]
    if best is None:
      best = a + 1
      if not see(a, best): unverified = True
    kept.append(best)
    a = best
  return kept, unverified


def shortcut_one(sdf, start, goal, cells, num_cells, th_in, n, clearance, check_step, path_cap, vertex_cap, lookahead, x_lims=(-5.0, 5.0), y_lims=(-5.0, 5.0),
                 total_time_sec=10.0):
  """one problem -> dict(th (n,4), vertex_index (vertex_cap) int32, num_vertices, length, info)"""
  H, W = sdf.shape
  L = int(num_cells)
  info = (BIT_NO_PATH if L <= 0 else 0) | (BIT_INPUT_TRUNCATED if L > path_cap else 0)
  vi = np.full(vertex_cap, -1, np.int32)
  if info: return dict(th=np.array(th_in, np.float64), vertex_index=vi, num_vertices=0, length=-1.0, info=info)
  start, goal = (float(start[0]), float(start[1])), (float(goal[0]), float(goal[1]))
  V = vertices_of(cells[:L], start, goal, W, x_lims, y_lims)
  kept, unverified = greedy(sdf, V, float(clearance), float(check_step), int(lookahead), x_lims, y_lims)
  th, S = PA.resample([V[k] for k in kept], n, start, goal, total_time_sec)
  m = len(kept)
  if m > vertex_cap: info |= BIT_VERTEX_TRUNCATED
  if unverified: info |= BIT_UNVERIFIED
  vi[:min(m, vertex_cap)] = kept[:vertex_cap]
  return dict(th=th, vertex_index=vi, num_vertices=m, length=S, info=info)


def shortcut_paths(sdfs, start, goal, path_cells, num_cells, th_in, n, clearance, check_step, path_cap, vertex_cap, lookahead=1 << 30, env_index=None, **kw):
  """sdfs (E,H,W) (E = 1: shared), start / goal (B,1,4), path_cells (B,path_cap), num_cells (B), th_in (B,n,4) -> dict of stacked arrays, as dgp_shortcut_paths
  writes them"""
  sdfs = np.asarray(sdfs)
  B = start.shape[0]
  rs = []
  for b in range(B):
    e = int(env_index[b]) if env_index is not None else (b if sdfs.shape[0] > 1 else 0)
    rs.append(shortcut_one(sdfs[e], start[b, 0, :2], goal[b, 0, :2], path_cells[b], num_cells[b], th_in[b], n, clearance, check_step, path_cap, vertex_cap, lookahead, **kw))
  out = {k: np.stack([r[k] for r in rs]) for k in ('th', 'vertex_index')}
  out['num_vertices'] = np.array([r['num_vertices'] for r in rs], np.int32)
  out['info'] = np.array([r['info'] for r in rs], np.int32)
  out['length'] = np.array([r['length'] for r in rs], np.float64)
  return out
