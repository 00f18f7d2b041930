"""Plain numpy / Python fp64 restatement of dgp_init_paths (include/dgpmp2_hip.h), written independently of the kernel: the sweep rule stated literally (a row's closure
is the minimum over every cell of its run, formed as a matrix; no scan, no carry), an independent heap-based Dijkstra over the same 5-7 moves that the swept field must
equal wherever it converged, the greedy trace, and the resampling of the polyline in Python floats (IEEE binary64, never contracted).  The path itself has no
counterpart in the reference (its RRT* is randomised and OMPL is not part of this build); what has one is the validity rule -- a cell is free where its stored
distance exceeds the clearance, Env2D.is_feasible -- and the velocities of path_to_traj_avg_vel (utils/planner_utils.py:60-71).
tests/test_paths_oracle.py holds this file against itself and against the feasibility property; tests/test_hip_paths.py holds the kernel against this file."""
import functools
import heapq
import math

import numpy as np

import problems_oracle as PO

INF = 0xffffffff
NEIGHBOURS = ((0, 1), (-1, 0), (0, -1), (1, 0), (-1, 1), (-1, -1), (1, -1), (1, 1))      # the order of the trace, (dr, dc)
BIT_START, BIT_GOAL, BIT_UNREACHABLE, BIT_UNCONVERGED, BIT_TRUNCATED = 1, 2, 4, 8, 16


def geometry(W, x_lims, y_lims):
  res = (x_lims[1] - x_lims[0]) / (W * 1.)
  return res, (0 - x_lims[0] / res), (0 - y_lims[0] / res)      # res, orig_x, orig_y: the lookup's (problems_oracle.signed_distance)


def cell_of(x, y, H, W, x_lims, y_lims):
  res, ox, oy = geometry(W, x_lims, y_lims)
  px, py = ox + float(x) / res, oy - float(y) / res
  return int(min(max(math.floor(py + 0.5), 0), H - 1)), int(min(max(math.floor(px + 0.5), 0), W - 1))      # (r, c)


def point_of(r, c, W, x_lims, y_lims):
  res, ox, oy = geometry(W, x_lims, y_lims)
  return (float(c) - ox) * res, (oy - float(r)) * res


def free_cells(sdf, clearance):
  return np.asarray(sdf).astype(np.float64) > float(clearance)


def move_allowed(free, r, c, dr, dc):
  """the move (r, c) -> (r + dr, c + dc): inside the grid, both ends free, and for a diagonal both cells that share its corner free"""
  H, W = free.shape
  nr, nc = r + dr, c + dc
  if not (0 <= nr < H and 0 <= nc < W) or not (free[r, c] and free[nr, nc]): return False
  return not (dr and dc) or (free[nr, c] and free[r, nc])


@functools.lru_cache(maxsize=None)
def _steps(n):
  k = np.arange(n)
  return 5 * np.abs(k[:, None] - k[None, :])      # 5 |c - k|


def _close(row, free_row):
  """the closure of one row, in place: every free cell c <- min_k (row[k] + 5 |c - k|) over the cells k of its maximal run of free cells"""
  W = len(row)
  c = 0
  while c < W:
    if not free_row[c]:
      c += 1
      continue
    e = c
    while e < W and free_row[e]: e += 1
    m = row[c:e][None, :] + _steps(e - c)      # (int64; an INF entry stays >= INF)
    row[c:e] = np.minimum(m.min(1), INF)
    c = e


def _pass(D, free, rows, step):
  H, W = D.shape
  for r in rows:
    p = r - step      # the row this pass has already finished
    if 0 <= p < H:
      # every free cell of row r: the minimum of itself and the allowed moves from row p (a whole row at a time; move_allowed states the rule for one move)
      src = np.where(free[p], D[p], INF)                    # what a cell of row p offers
      best = np.minimum(D[r], np.minimum(src + 5, INF))     # the axis move from (p, c)
      both = free[p] & free[r]                              # column c: (p, c) and (r, c) free
      ok = both[1:] & both[:-1]                             # columns c - 1 and c: the two ends of either diagonal and the two cells on its corner
      best[1:] = np.where(ok, np.minimum(best[1:], np.minimum(src[:-1] + 7, INF)), best[1:])      # from (p, c - 1)
      best[:-1] = np.where(ok, np.minimum(best[:-1], np.minimum(src[1:] + 7, INF)), best[:-1])    # from (p, c + 1)
      D[r] = np.where(free[r], best, D[r])
    _close(D[r], free[r])


def sweep_field(free, goal_cell, max_sweeps):
  """-> (D (H,W) uint32, sweeps run, converged: the last sweep changed no cell)"""
  H, W = free.shape
  D = np.full((H, W), INF, np.int64)
  if free[goal_cell]: D[goal_cell] = 0
  sweeps, converged = 0, False
  while sweeps < max_sweeps and not converged:
    before = D.copy()
    _pass(D, free, range(H), 1)                # down
    _pass(D, free, range(H - 1, -1, -1), -1)   # up
    sweeps += 1
    converged = bool(np.array_equal(before, D))
  return D.astype(np.uint32), sweeps, converged


def dijkstra_field(free, goal_cell):
  """the 5-7 shortest-path field from a heap: every cell's cost to the goal over allowed moves (the move rule is symmetric)"""
  H, W = free.shape
  D = np.full((H, W), INF, np.int64)
  if not free[goal_cell]: return D.astype(np.uint32)
  D[goal_cell] = 0
  heap = [(0, goal_cell[0], goal_cell[1])]
  while heap:
    d, r, c = heapq.heappop(heap)
    if d > D[r, c]: continue
    for dr, dc in NEIGHBOURS:
      if move_allowed(free, r, c, dr, dc):
        nd = d + (7 if dr and dc else 5)
        if nd < D[r + dr, c + dc]:
          D[r + dr, c + dc] = nd
          heapq.heappush(heap, (nd, r + dr, c + dc))
  return D.astype(np.uint32)


def trace(D, free, start_cell):
  """-> the traced cells [(r, c)], the start cell first"""
  H, W = D.shape
  r, c = start_cell
  cells = [(r, c)]
  while int(D[r, c]) > 0 and len(cells) < H * W:
    for dr, dc in NEIGHBOURS:
      nr, nc = r + dr, c + dc
      if move_allowed(free, r, c, dr, dc) and int(D[nr, nc]) != INF and int(D[nr, nc]) + (7 if dr and dc else 5) == int(D[r, c]):
        r, c = nr, nc
        break
    else:
      break
    cells.append((r, c))
  return cells


def resample(vertices, n, start, goal, total_time_sec):
  """vertices: V_0 .. V_{L+1} as (x, y) -> (th (n, 4), S)"""
  L1 = len(vertices) - 1
  seg, s = [], [0.0]
  for j in range(L1):
    dx, dy = vertices[j + 1][0] - vertices[j][0], vertices[j + 1][1] - vertices[j][1]
    seg.append(math.sqrt(dx * dx + dy * dy))
    s.append(s[-1] + seg[-1])
  S, N = s[-1], n - 1
  th = np.zeros((n, 4))
  for i in range(n):
    if i == N: x, y = goal
    else:
      t = S * i / N
      j = next((j for j in range(L1) if s[j + 1] >= t), L1 - 1)
      f = (t - s[j]) / seg[j] if seg[j] > 0 else 0.0
      x = vertices[j][0] + f * (vertices[j + 1][0] - vertices[j][0])
      y = vertices[j][1] + f * (vertices[j + 1][1] - vertices[j][1])
    th[i] = x, y, (goal[0] - start[0]) / total_time_sec, (goal[1] - start[1]) / total_time_sec
  return th, S


def init_path_one(sdf, start, goal, n, clearance, max_sweeps, path_cap, x_lims=(-5.0, 5.0), y_lims=(-5.0, 5.0), total_time_sec=10.0):
  """one problem -> dict(th_init (n,4), field (H,W) uint32, path_cells (path_cap) int32, num_cells, length, info, sweeps)"""
  H, W = sdf.shape
  start, goal = (float(start[0]), float(start[1])), (float(goal[0]), float(goal[1]))
  free = free_cells(sdf, clearance)
  sc, gc = cell_of(start[0], start[1], H, W, x_lims, y_lims), cell_of(goal[0], goal[1], H, W, x_lims, y_lims)
  D, sweeps, converged = sweep_field(free, gc, max_sweeps)
  info = (0 if free[sc] else BIT_START) | (0 if free[gc] else BIT_GOAL)
  if not converged: info |= BIT_UNCONVERGED
  elif int(D[sc]) == INF: info |= BIT_UNREACHABLE
  cells = []
  if info:
    th = PO.straight_line(start, goal, n, total_time_sec)
    dx, dy = goal[0] - start[0], goal[1] - start[1]
    L, S = 0, math.sqrt(dx * dx + dy * dy)
  else:
    cells = trace(D, free, sc)
    L = len(cells)
    th, S = resample([start] + [point_of(r, c, W, x_lims, y_lims) for r, c in cells] + [goal], n, start, goal, total_time_sec)
    if L > path_cap: info |= BIT_TRUNCATED
  cells_out = np.full(path_cap, -1, np.int32)
  cells_out[:min(L, path_cap)] = [r * W + c for r, c in cells[:path_cap]]
  return dict(th_init=th, field=D, path_cells=cells_out, num_cells=L, length=S, info=info, sweeps=sweeps)


def init_paths(sdfs, start, goal, n, clearance, max_sweeps, path_cap, env_index=None, **kw):
  """sdfs (E,H,W) (E = 1: shared), start / goal (B,1,4) -> dict of stacked arrays, as dgp_init_paths writes them"""
  sdfs = np.asarray(sdfs)
  B = start.shape[0]
  rs = []
  for b in range(B):
    e = int(env_index[b]) if env_index is not None else (b if sdfs.shape[0] > 1 else 0)
    rs.append(init_path_one(sdfs[e], start[b, 0, :2], goal[b, 0, :2], n, clearance, max_sweeps, path_cap, **kw))
  out = {k: np.stack([r[k] for r in rs]) for k in ('th_init', 'field', 'path_cells')}
  out['num_cells'] = np.array([r['num_cells'] for r in rs], np.int32)
  out['info'] = np.array([r['info'] for r in rs], np.int32)
  out['length'] = np.array([r['length'] for r in rs], np.float64)
  out['sweeps'] = np.array([r['sweeps'] for r in rs], np.int32)
  return out
