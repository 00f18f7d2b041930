"""CPU-only tests of the shortcut oracle (tests/shortcut_oracle.py) and of the host side of dgp_shortcut_paths.

The reference's simplifySolution is OMPL's and randomised: there is no fixture from it.  What pins the rule instead, on every case of tests/shortcut_cases.py:
  * every kept segment is visible, or joins adjacent vertices with bit 3 set; no later candidate inside the lookahead is visible (maximality) -- both re-checked
    with a separately written, vectorised `visible` (numpy over all check points of a segment at once, its own bilinear lookup);
  * k_0 = 0, k_last = L + 1, strictly increasing; the new length lies between the straight distance and the grid path's; row 0 is the start, row N the goal, the
    velocities are path_to_traj_avg_vel's;
  * the cases take every branch the rule has (the counts are asserted);
  * the feasibility property on the sampled problems: no flag, a dense resample of the new polyline above clearance - check_step (the bound the header derives),
    the n states above the clearance;
  * argument validation of dgp_shortcut_paths (nothing touches a device), the struct layout and the Python front end's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import paths_cases as PC
import paths_oracle as PA
import problems_oracle as PO
import shortcut_cases as SC
import shortcut_oracle as SO
from dgpmp2_amd import _capi


# ---- a second `visible`, vectorised, sharing no code with the oracle's ------------------------------------------------------------------------------------------------

def _distances(sdf, x, y, x_lims, y_lims):
  """env_2d.py:119-175 for arrays of points (numpy float64 elementwise arithmetic is IEEE binary64, never contracted)"""
  H, W = sdf.shape
  res = (x_lims[1] - x_lims[0]) / (W * 1.)
  px, py = (0 - x_lims[0] / res) + x / res, (0 - y_lims[0] / res) - y / res
  x1, y1 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
  x2, y2 = np.clip(x1 + 1, 0, W - 1), np.clip(y1 + 1, 0, H - 1)
  x1, y1 = np.clip(x1, 0, W - 1), np.clip(y1, 0, H - 1)
  d = ((x2 - px) * (y2 - py)) * sdf[y1, x1] + ((px - x1) * (y2 - py)) * sdf[y1, x2] + ((x2 - px) * (py - y1)) * sdf[y2, x1] + ((px - x1) * (py - y1)) * sdf[y2, x2]
  inside = (x <= x_lims[1]) & (x >= x_lims[0]) & (y <= y_lims[1]) & (y >= y_lims[0])
  return np.where(inside, d, x_lims[1] - x_lims[0])


def _visible(sdf, P, Q, clearance, check_step, x_lims, y_lims):
  dx, dy = Q[0] - P[0], Q[1] - P[1]
  m = max(abs(dx), abs(dy)) / check_step      # (no NaN in these cases)
  assert m <= 2.0 ** 20
  M = int(np.ceil(m)) if m > 1 else 1
  f = np.arange(M + 1, dtype=np.float64) / np.float64(M)
  return bool((_distances(sdf, P[0] + f * dx, P[1] + f * dy, x_lims, y_lims) > clearance).all())


def _problems(name, io='f64', **kw):
  g = SC.group(name)
  out, prm = SC.expected(name, io, **kw)
  inp, _ = SC.inputs(name, io)
  for b, case in enumerate(g.names):
    yield g, b, case, {k: v[b] for k, v in inp.items()}, {k: v[b] for k, v in out.items()}, prm


def _vertices(g, b, i, io='f64'):
  s, t = PC._round(g.start, io)[b, 0, :2], PC._round(g.goal, io)[b, 0, :2]
  return SO.vertices_of(i['path_cells'][:i['num_cells']], s, t, g.W, g.x_lims, g.y_lims)


@pytest.mark.parametrize('name', SC.GROUPS)
def test_kept_segments_are_visible_and_maximal(name):
  for g, b, case, i, o, prm in _problems(name):
    if o['info'] & 3: continue
    sdf, V = g.sdfs[g.env[b]], _vertices(g, b, i)
    see = lambda p, q: _visible(sdf, V[p], V[q], g.clearance, prm['check_step'], g.x_lims, g.y_lims)
    k = [int(v) for v in o['vertex_index'][:o['num_vertices']]]
    assert k[0] == 0 and k[-1] == len(V) - 1 == i['num_cells'] + 1 and all(q > p for p, q in zip(k[:-1], k[1:])), case
    forced = 0
    for p, q in zip(k[:-1], k[1:]):
      if not see(p, q):
        assert q == p + 1, (case, p, q)
        forced += 1
      hi = min(len(V) - 1, p + prm['lookahead'])
      assert not any(see(p, j) for j in range(max(q, p + 1) + 1, hi + 1)), (case, p, q)      # no later candidate is visible
    assert (forced > 0) == bool(o['info'] & SO.BIT_UNVERIFIED), case


@pytest.mark.parametrize('name', SC.GROUPS)
def test_lengths_and_trajectory(name):
  for g, b, case, i, o, prm in _problems(name):
    s, t = g.start[b, 0, :2], g.goal[b, 0, :2]
    if o['info'] & 3:
      assert o['num_vertices'] == 0 and (o['vertex_index'] == -1).all() and o['length'] == -1.0 and np.array_equal(o['th'], i['th_init']), case
      continue
    assert o['length'] <= i['length'] * (1 + 1e-12) and o['length'] >= np.sqrt(((t - s) ** 2).sum()) * (1 - 1e-12), case
    th = o['th']
    assert np.array_equal(th[0, :2], s) and np.array_equal(th[-1, :2], t), case      # row 0 is the start, row N the goal
    assert np.array_equal(th[:, 2:], np.tile((t - s) / g.t_sec, (g.n, 1))), case
    assert (o['vertex_index'][o['num_vertices']:] == -1).all(), case


def test_cases_take_every_branch():
  info = {(name, c): int(v) for name in SC.GROUPS for c, v in zip(SC.group(name).names, SC.expected(name)[0]['info'])}
  # bit 0: the three fallbacks of g16, and nothing else
  assert sorted(k[1] for k, v in info.items() if v & SO.BIT_NO_PATH) == ['enclosed_goal', 'goal_blocked', 'start_blocked']
  assert all(v == SO.BIT_NO_PATH for v in info.values() if v & SO.BIT_NO_PATH)
  # bit 3: every path with a vertex on the last column, where the lookup collapses: the corridor of s16 both ways (forced segment after forced segment), the goal
  # on the last column of g24, the tooth of g100 on its last but one column
  assert sorted(k for k, v in info.items() if v & SO.BIT_UNVERIFIED) == [('g100', 'serpentine_ragged'), ('g100', 'serpentine_ragged_back'), ('g24', 'goal_last_row_and_column'),
                                                                         ('s16', 'corridor_last_column'), ('s16', 'corridor_last_column_back')]
  s16, o16 = SC.group('s16'), SC.expected('s16')[0]
  b = s16.names.index('corridor_last_column')
  k = o16['vertex_index'][b][:o16['num_vertices'][b]]
  assert o16['num_vertices'][b] == 15 and (np.diff(k)[1:] == 1).all() and np.diff(k)[0] > 1      # one shortcut to the gap, then cell by cell down the corridor
  # the start outside the limits: its cell is column 0 (once by the clamp), its check points left of the limits are feasible (MAX_D), the path is simplified
  for case, clamped in (('start_hair_outside', False), ('start_outside_cell_clamps', True)):
    b = s16.names.index(case)
    x, y = s16.start[b, 0, :2]
    res, ox, oy = PA.geometry(16, s16.x_lims, s16.y_lims)
    assert x < s16.x_lims[0] and PO.signed_distance(s16.sdfs[0], x, y, s16.x_lims, s16.y_lims) == 10.0
    assert (np.floor(ox + x / res + 0.5) < 0) == clamped and SC.inputs('s16')[0]['path_cells'][b][0] % 16 == 0
    assert info[('s16', case)] == 0 and o16['num_vertices'][b] == 4 and o16['vertex_index'][b][1] > 1
  # bit 1: path_cap below L truncates the input: untouched; bit 2: vertex_cap below m truncates vertex_index only
  g24, o24 = SC.group('g24'), SC.expected('g24')[0]
  cut, _ = SC.expected('g24', 'f64', SC.ALL, 5, 4)
  assert (cut['info'] == SO.BIT_INPUT_TRUNCATED).all() and (cut['num_vertices'] == 0).all() and np.array_equal(cut['th'], SC.inputs('g24')[0]['th_init'])
  few, _ = SC.expected('g24', 'f64', SC.ALL, None, 2)
  assert np.array_equal(few['info'], o24['info'] | np.where(o24['num_vertices'] > 2, SO.BIT_VERTEX_TRUNCATED, 0)) and ((few['info'] & SO.BIT_VERTEX_TRUNCATED) != 0).sum() == 3
  assert np.array_equal(few['vertex_index'], o24['vertex_index'][:, :2]) and np.array_equal(few['th'], o24['th']) and np.array_equal(few['num_vertices'], o24['num_vertices'])
  # lookahead = 3 changes the serpentine's result: more vertices, a longer polyline
  g64, o64 = SC.group('g64'), SC.expected('g64')[0]
  la3, _ = SC.expected('g64', 'f64', 3)
  b = g64.names.index('serpentine')
  assert o64['num_vertices'][b] == 12 and la3['num_vertices'][b] >= (237 + 1) // 3 + 1 > 12 and la3['length'][b] > o64['length'][b]
  assert (np.diff(la3['vertex_index'][b][:la3['num_vertices'][b]]) <= 3).all()
  # more vertices than two trips of 64 candidates, and a segment with more than 64 check points
  for name in ('g100', 'g256'):
    g, (o, prm), (inp, _) = SC.group(name), SC.expected(name), SC.inputs(name)
    assert inp['num_cells'].max() + 2 > 128, name
    longest = 0
    for b in range(len(g.names)):
      V = SC.kept_vertices(name, b, o)
      longest = max([longest] + [len(SO.check_points(p, q, prm['check_step'])) for p, q in zip(V[:-1], V[1:])])
    assert longest > 64, name
  # start and goal on one cell point: two vertices, S = 0, every row the start
  g16, o16g = SC.group('g16'), SC.expected('g16')[0]
  b = g16.names.index('same_point_on_cell')
  assert o16g['num_vertices'][b] == 2 and o16g['length'][b] == 0 and (o16g['th'][b][:, :2] == g16.start[b, 0, :2]).all()
  # strictly shorter than the grid path: everywhere but there
  shorter = sum(int(o['length'] < i['length']) for name in SC.GROUPS for g, b, case, i, o, prm in _problems(name) if not o['info'] & 3)
  assert shorter == sum(len(SC.group(name).names) for name in SC.GROUPS) - 3 - 1
  # fp32 tensors see a rounded grid and rounded points: the discrete results of these cases do not move
  for name in SC.GROUPS:
    a, b32 = SC.expected(name)[0], SC.expected(name, 'f32')[0]
    assert np.array_equal(a['info'], b32['info']) and np.array_equal(a['vertex_index'], b32['vertex_index']), name


@pytest.mark.parametrize('name', SC.PROPERTY_GROUPS)
def test_feasibility_property(name):
  """info == 0 => the whole polyline stays above clearance - check_step: every check point of a visible segment is above the clearance, consecutive check points are at
  most check_step apart in each coordinate, and the bilinear interpolant of a distance transform changes by at most |dx| + |dy| (include/dgpmp2_hip.h).  The n states
  are held to the clearance itself, which the bound does not promise: on these ten problems the dense minimum stays above it (the worst by 0.059 cells)."""
  g = SC.group(name)
  out, prm = SC.expected(name)
  assert (out['info'] == 0).all()
  worst = np.inf
  for b in range(len(g.names)):
    sdf = g.sdfs[g.env[b]]
    d = _distances(sdf, out['th'][b][:, 0], out['th'][b][:, 1], g.x_lims, g.y_lims)
    assert (d > g.clearance).all(), (name, b, d.min())
    dense = PA.resample(SC.kept_vertices(name, b, out), 40 * g.n, g.start[b, 0, :2], g.goal[b, 0, :2], g.t_sec)[0]
    dd = min(PO.signed_distance(sdf, x, y, g.x_lims, g.y_lims) for x, y in dense[:, :2])
    assert dd > g.clearance - prm['check_step'], (name, b, dd)
    worst = min(worst, dd)
  print('%s: dense minimum %.6f above the clearance (%.3f cells)' % (name, worst - g.clearance, (worst - g.clearance) / (4 * prm['check_step'])))


# ---- the entry point, without a GPU -------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def api():
  if not os.path.exists(_capi.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _capi.get_api()


def _cfg(**kw):
  base = dict(num_states=16, dof=2, io_dtype=_capi.DGP_F64, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4,
              Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4)
  base.update(kw)
  return _capi.make_config(**base)


def test_struct_layout_and_symbol(api):
  P = _capi.DgpShortcutParams
  assert C.sizeof(P) == 32      # include/dgpmp2_hip.h: two doubles, four int32
  assert [getattr(P, f).offset for f in ('clearance', 'check_step', 'path_cap', 'vertex_cap', 'lookahead', 'reserved')] == [0, 8, 16, 20, 24, 28]
  assert 'shortcut_paths' in _capi.CApi.SYMBOLS and api.shortcut_paths is not None and api.abi_version() == 7
  p = _capi.Solver.shortcut_params(0.8, 0.1, 40)
  assert (p.clearance, p.check_step, p.path_cap, p.vertex_cap, p.lookahead, p.reserved) == (0.8, 0.1, 40, 0, 1 << 30, 0)


def test_shortcut_paths_validates_arguments_without_gpu(api):
  s = _capi.Solver(_cfg())
  res = 10.0 / 16
  ok_sdf, ok = s.sdf_arg(0x1000, 16, 16, 0), s.shortcut_params(0.8, res / 4, 8, 4)
  call = lambda solver, sdf, p, batch=8, **kw: solver.shortcut_paths(batch, sdf, p, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, **kw)

  def refused(*a, **kw):
    with pytest.raises(_capi.DgpError) as e:
      call(*a, **kw)
    assert len(str(e.value)) > 20 and e.value.code == _capi.DGP_EINVAL
    return e.value
  s3 = _capi.Solver(_cfg(dof=3, Q_c_inv=[[1, 0, 0], [0, 1, 0], [0, 0, 1]]))
  assert 'dof' in str(refused(s3, ok_sdf, ok))
  refused(s, ok_sdf, None)                                       # NULL params
  refused(s, None, ok)                                           # NULL sdf
  refused(s, s.sdf_arg(None, 16, 16, 0), ok)                     # ... or no grid in it
  assert 'row-major' in str(refused(s, s.sdf_arg(0x1000, 16, 16, 0, layout=_capi.DGP_SDF_TILED4), ok))      # tiled grids are refused
  refused(s, s.sdf_arg(0x1000, 16, 16, 0, layout=7), ok)
  for rows, cols in ((4097, 16), (16, 4097), (0, 16), (16, 0)): refused(s, s.sdf_arg(0x1000, rows, cols, 0), ok)
  refused(s, s.sdf_arg(0x1000, 16, 16, -256), ok)               # a negative batch stride
  assert 'NaN' in str(refused(s, ok_sdf, s.shortcut_params(float('nan'), res / 4, 8, 4)))
  for bad in (float('nan'), float('inf'), -float('inf'), 0.0, -1.0, res / 16 * (1 - 1e-12)):
    assert 'check_step' in str(refused(s, ok_sdf, s.shortcut_params(0.8, bad, 8, 4))), bad
  for bad in (0, -1, (1 << 18) + 1):
    assert 'path_cap' in str(refused(s, ok_sdf, s.shortcut_params(0.8, res / 4, bad, 4))), bad
  assert 'vertex_cap' in str(refused(s, ok_sdf, s.shortcut_params(0.8, res / 4, 8, -1)))
  for bad in (0, -3):
    assert 'lookahead' in str(refused(s, ok_sdf, s.shortcut_params(0.8, res / 4, 8, 4, bad))), bad
  assert 'vertex_cap' in str(refused(s, ok_sdf, s.shortcut_params(0.8, res / 4, 8, 0), vertex_index=0x1000))      # vertex_index without room for it
  refused(s, ok_sdf, ok, batch=0); refused(s, ok_sdf, ok, batch=-2)

  def raw(h, start=0x1000, goal=0x1000, cells=0x1000, num=0x1000, th=0x1000):
    return api.shortcut_paths(h, 8, C.byref(ok_sdf), None, C.byref(ok), start, goal, cells, num, th, None, None, None, None, None)
  assert raw(None) == _capi.DGP_EINVAL and b'null handle' in api.last_error()
  for kw in (dict(start=None), dict(goal=None), dict(cells=None), dict(num=None), dict(th=None)):
    assert raw(s.handle, **kw) == _capi.DGP_EINVAL, kw
  # a request of dgp_time_next_launch does not survive a rejected call
  assert api.time_next_launch(0x10, 0x20) == _capi.DGP_OK
  assert raw(None) == _capi.DGP_EINVAL
  refused(s, ok_sdf, ok, batch=0)      # (a surviving request would make no difference here: nothing is launched; the GPU test times a launch)
  assert api.time_next_launch(None, None) == _capi.DGP_OK


class _FakeCuda(object):
  """a tensor that says it lives on the device: the argument checks are all that read it here"""

  def __new__(cls, *shape):
    import torch

    class T(torch.Tensor):
      @property
      def is_cuda(self): return True
    return torch.zeros(*shape).as_subclass(T)


def test_front_end_refusals_and_info():
  import torch
  from dgpmp2_amd import datasets as D
  from dgpmp2_amd.datasets import problem_generation as PG
  assert D.shortcut_paths is PG.shortcut_paths and D.ShortcutInfo is PG.ShortcutInfo
  z, th = torch.zeros(1, 1, 4), torch.zeros(1, 8, 4)
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    PG.shortcut_paths(object(), torch.zeros(1, 1, 16, 16), z, z, th, None)
  with pytest.raises(RuntimeError, match='th_initb.*CUDA/ROCm'):
    PG.shortcut_paths(object(), _FakeCuda(1, 1, 16, 16), _FakeCuda(1, 1, 4), _FakeCuda(1, 1, 4), th, None)
  with pytest.raises(ValueError, match='untile.*row-major'):      # a TiledSdf is refused, with the way out
    PG.shortcut_paths(object(), _FakeCuda(1, 1, 4, 4, 4, 4), _FakeCuda(1, 1, 4), _FakeCuda(1, 1, 4), _FakeCuda(1, 8, 4), None)
  no_cells = PG.PathInfo(torch.zeros(1, dtype=torch.int32), None, None)      # the positional constructor of before still works
  assert no_cells.shortcut is None and no_cells.path_cells is None
  with pytest.raises(ValueError, match='path_cap'):
    PG.shortcut_paths(object(), _FakeCuda(1, 1, 16, 16), _FakeCuda(1, 1, 4), _FakeCuda(1, 1, 4), _FakeCuda(1, 8, 4), no_cells)
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    PG.init_paths(object(), torch.zeros(1, 1, 16, 16), z, z, shortcut=True)
  with pytest.raises(ValueError, match='init'):
    PG.generate_dataset('unused', 'train', _FakeCuda(2, 16, 16), None, 1, init='rrt_star')
  # 'shortcut_path' is an accepted value: the refusal that follows is about the host tensor
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    PG.sample_problems(object(), torch.zeros(1, 1, 16, 16), init='shortcut_path')
  assert 'shortcut_path' in PG.INITS
  info = PG.ShortcutInfo(torch.tensor([0, 1, 2, 4, 8, 12], dtype=torch.int32), None, None)
  assert info.simplified.tolist() == [True, False, False, True, True, True] and info.vertex_index is None
  assert info.unverified.tolist() == [False, False, False, False, True, True] and info.input_truncated.tolist() == [False, False, True, False, False, False]
