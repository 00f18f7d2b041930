"""Inputs of the shortcut tests (tests/test_shortcut_oracle.py, tests/test_hip_shortcut.py): the groups of tests/paths_cases.py with the grid paths the path oracle
traced for them (paths_cases.expected) as input, one small group of their own, and the shortcut oracle's answer (tests/shortcut_oracle.py), computed once per
(group, io, parameters) and shared read-only.
  s16   16 x 16   a block in the middle of the map with a start OUTSIDE x_lims -- a hair (1e-9: the cell is column 0 without a clamp) and by more than half a cell
                  (the cell clamps to column 0); every check point left of the limits returns MAX_D and is feasible, as in the reference --
                  and a corridor one cell wide along the LAST column behind a wall with one gap: the reference's lookup collapses to 0 on the last column (clamped
                  taps), so no segment that ends on a cell point of the corridor is visible -- the adjacent segments are forced, bit 3.
check_step is a quarter of a cell (the front end's default) unless a test says otherwise; fp32 follows the convention of paths_cases._round: grids and points are
rounded once on the way in, and so is the trajectory that comes in."""
import functools

import numpy as np

import paths_cases as PC
import paths_oracle as PA
import shortcut_oracle as SO

GROUPS = PC.GROUPS + ('s16',)
PROPERTY_GROUPS = PC.PROPERTY_GROUPS
ALL = 1 << 30      # lookahead: no bound


@functools.lru_cache(maxsize=None)
def group(name):
  if name != 's16': return PC.group(name)
  H = W = 16
  at = lambda r, c, off=(0.013, -0.021): PC._at(r, c, W, PC.LIMS, PC.LIMS, off)
  block, corridor = np.ones((H, W)), np.ones((H, W))
  block[5:11, 6:10] = 0.0
  corridor[:, 14] = 0.0; corridor[2, 14] = 1.0
  y8 = at(8, 0)[1]
  return PC._group(name, [block, corridor], 9, [
      ('start_hair_outside', 0, (-5.0 - 1e-9, y8), at(8, 13)), ('start_outside_cell_clamps', 0, (-5.4, y8), at(8, 13)), ('block_inside', 0, at(8, 2), at(8, 13)),
      ('corridor_last_column', 1, at(3, 4), at(13, 15)), ('corridor_last_column_back', 1, at(13, 15), at(3, 4))])


@functools.lru_cache(maxsize=None)
def inputs(name, io='f64'):
  """What dgp_init_paths gives for the group (the path oracle's answer) -> (dict with th_init, path_cells, num_cells, info, length, path_cap)"""
  if name != 's16': out, _, cap = PC.expected(name, io)
  else:
    g = group(name)
    free_run = PA.init_paths(PC._round(g.sdfs, io), PC._round(g.start, io), PC._round(g.goal, io), g.n, g.clearance, 64, 1 << 10, env_index=g.env, x_lims=g.x_lims,
                             y_lims=g.y_lims, total_time_sec=g.t_sec)
    assert not free_run['info'].any()
    cap = int(free_run['num_cells'].max()) + 3
    out = dict(free_run, path_cells=np.ascontiguousarray(free_run['path_cells'][:, :cap]))
  out = dict(out, th_init=PC._round(out['th_init'], io))      # (what a tensor of the io dtype holds)
  for a in out.values(): a.setflags(write=False)
  return out, cap


def check_step_of(g):
  return 0.25 * (g.x_lims[1] - g.x_lims[0]) / g.W


@functools.lru_cache(maxsize=None)
def expected(name, io='f64', lookahead=ALL, path_cap=None, vertex_cap=None, check_step=None):
  """The shortcut oracle's answer for a group as the kernel sees it with `io` tensors -> (dict, params: dict(path_cap, vertex_cap, lookahead, check_step)).
  path_cap None: that of inputs(); a smaller one truncates the INPUT (the first path_cap columns of path_cells: bit 1).  vertex_cap None: the most vertices kept
  plus 2."""
  g = group(name)
  inp, cap = inputs(name, io)
  if check_step is None: check_step = check_step_of(g)
  if path_cap is None: path_cap = cap
  cells = np.ascontiguousarray(inp['path_cells'][:, :path_cap])
  run = lambda vcap: SO.shortcut_paths(PC._round(g.sdfs, io), PC._round(g.start, io), PC._round(g.goal, io), cells, inp['num_cells'], inp['th_init'], g.n, g.clearance,
                                       check_step, path_cap, vcap, lookahead, env_index=g.env, x_lims=g.x_lims, y_lims=g.y_lims, total_time_sec=g.t_sec)
  if vertex_cap is None:
    full, _ = expected(name, io, lookahead, path_cap, path_cap + 2, check_step)      # (every vertex fits)
    vertex_cap = int(full['num_vertices'].max()) + 2
    out = dict(full, vertex_index=np.ascontiguousarray(full['vertex_index'][:, :vertex_cap]))
  else:
    out = run(vertex_cap)
  for a in out.values(): a.setflags(write=False)
  return out, dict(path_cap=path_cap, vertex_cap=vertex_cap, lookahead=lookahead, check_step=check_step)


def kept_vertices(name, b, out, io='f64'):
  """the kept vertices of problem b as (x, y) tuples (needs every kept index inside vertex_cap)"""
  g = group(name)
  inp, _ = inputs(name, io)
  s, t = PC._round(g.start, io)[b, 0, :2], PC._round(g.goal, io)[b, 0, :2]
  V = SO.vertices_of(inp['path_cells'][b][:inp['num_cells'][b]], s, t, g.W, g.x_lims, g.y_lims)
  return [V[k] for k in out['vertex_index'][b][:out['num_vertices'][b]]]
