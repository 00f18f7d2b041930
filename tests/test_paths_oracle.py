"""CPU-only tests of the initial-path oracle (tests/paths_oracle.py) and of the host side of dgp_init_paths.

The path has no fixture from the reference (its RRT* is randomised, OMPL is not part of this build).  What pins the rule instead:
  * wherever the literal sweep rule converged, its field equals an independent heap-based 5-7 Dijkstra cell for cell -- on every case of tests/paths_cases.py;
  * the trace ends in the goal cell at the cost D[start], over free cells only, no diagonal step cutting a corner; row 0 is the start, row N the goal, the velocities
    are path_to_traj_avg_vel's;
  * the feasibility property: with info == 0 every state of the trajectory has a bilinear distance (problems_oracle.signed_distance, the reference's lookup) above the
    clearance -- for start / goal pairs sampled at the sampler's default clearance (0.1 larger) on maps with cells of at most 0.07;
  * the cases take every branch the issue lists (the counts are asserted);
  * argument validation of dgp_init_paths (nothing touches a device), the struct layout and the Python front end's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import paths_cases as PC
import paths_oracle as PA
import problems_oracle as PO
from dgpmp2_amd import _capi


def _problems(name):
  g = PC.group(name)
  out, ms, cap = PC.expected(name)
  for b, case in enumerate(g.names):
    free = PA.free_cells(g.sdfs[g.env[b]], g.clearance)
    yield g, b, case, free, {k: v[b] for k, v in out.items()}


@pytest.mark.parametrize('name', PC.GROUPS)
def test_sweep_field_equals_dijkstra_wherever_it_converged(name):
  n = 0
  for g, b, case, free, o in _problems(name):
    if o['info'] & PA.BIT_UNCONVERGED: continue
    gc = PA.cell_of(g.goal[b, 0, 0], g.goal[b, 0, 1], g.H, g.W, g.x_lims, g.y_lims)
    assert np.array_equal(o['field'], PA.dijkstra_field(free, gc)), case
    assert (o['field'][~free] == PA.INF).all(), case
    n += 1
  assert n == len(PC.group(name).names)      # (every normal case converges inside its cap)


@pytest.mark.parametrize('name', PC.GROUPS)
def test_trace_and_trajectory(name):
  for g, b, case, free, o in _problems(name):
    s, goal, th = g.start[b, 0, :2], g.goal[b, 0, :2], o['th_init']
    assert np.array_equal(th[0, :2], s) and np.array_equal(th[-1, :2], goal), case      # row 0 is the start, row N the goal
    assert np.array_equal(th[:, 2:], np.tile((goal - s) / g.t_sec, (g.n, 1))), case
    if o['info'] & 15:
      assert o['num_cells'] == 0 and (o['path_cells'] == -1).all() and np.array_equal(th, PO.straight_line(s, goal, g.n, g.t_sec)), case
      assert o['length'] == np.sqrt((goal[0] - s[0]) ** 2 + (goal[1] - s[1]) ** 2)
      continue
    L = int(o['num_cells'])
    cells = [(int(v) // g.W, int(v) % g.W) for v in o['path_cells'][:L]]
    assert cells[0] == PA.cell_of(s[0], s[1], g.H, g.W, g.x_lims, g.y_lims) and cells[-1] == PA.cell_of(goal[0], goal[1], g.H, g.W, g.x_lims, g.y_lims), case
    assert (o['path_cells'][L:] == -1).all() and len(set(cells)) == L
    cost = 0
    for (r0, c0), (r1, c1) in zip(cells[:-1], cells[1:]):
      dr, dc = r1 - r0, c1 - c0
      assert max(abs(dr), abs(dc)) == 1 and PA.move_allowed(free, r0, c0, dr, dc), (case, (r0, c0), (r1, c1))      # free cells, no corner cut
      cost += 7 if dr and dc else 5
    assert cost == int(o['field'][cells[0]]), case
    # equal arc length: consecutive rows are no further apart than S / N, and the polyline's length is at least the straight distance
    step = np.sqrt((np.diff(th[:, :2], axis=0) ** 2).sum(1))
    assert step.max() <= o['length'] / (g.n - 1) * (1 + 1e-12) and o['length'] >= np.sqrt(((goal - s) ** 2).sum()) * (1 - 1e-12), case


def test_cases_take_every_branch():
  info = {c: int(i) for name in PC.GROUPS for c, i in zip(PC.group(name).names, PC.expected(name)[0]['info'])}
  assert info['enclosed_goal'] == PA.BIT_UNREACHABLE
  assert info['start_blocked'] == PA.BIT_START | PA.BIT_UNREACHABLE and info['goal_blocked'] == PA.BIT_GOAL | PA.BIT_UNREACHABLE
  assert all(v == 0 for c, v in info.items() if c not in ('enclosed_goal', 'start_blocked', 'goal_blocked'))
  g16, o16 = PC.group('g16'), PC.expected('g16')[0]
  i = g16.names.index('same_cell')
  assert o16['num_cells'][i] == 1 and o16['length'][i] > 0
  i = g16.names.index('same_point_on_cell')
  assert o16['num_cells'][i] == 1 and o16['length'][i] == 0 and (o16['th_init'][i][:, :2] == g16.start[i, 0, :2]).all()      # S == 0: every row is the start point
  # the diagonally touching cells: the straight diagonal step between them is refused, the path goes round
  i = g16.names.index('diagonal_touch')
  assert o16['num_cells'][i] > 2 and o16['field'][i][8, 7] > 7
  # the serpentine needs several sweeps, and one is not enough: bit 3, the straight line, the field as the single sweep left it
  g64, o64 = PC.group('g64'), PC.expected('g64')[0]
  assert o64['sweeps'].max() >= 4
  one, _, _ = PC.expected('g64', 'f64', 1, 240)
  i = g64.names.index('serpentine')
  assert one['info'][i] == PA.BIT_UNCONVERGED and one['num_cells'][i] == 0 and not np.array_equal(one['field'][i], o64['field'][i])
  assert np.array_equal(one['th_init'][i], PO.straight_line(g64.start[i, 0, :2], g64.goal[i, 0, :2], g64.n, g64.t_sec))
  # the U-shaped trap: the path first runs away from the goal
  i = g64.names.index('u_trap')
  cols = o64['path_cells'][i][:o64['num_cells'][i]] % 64
  assert cols[0] == 34 and cols.min() < 24 and cols[-1] == 52
  # path_cap smaller than L: bit 4 only truncates
  g24, o24 = PC.group('g24'), PC.expected('g24')[0]
  cut, _, _ = PC.expected('g24', 'f64', 5, 5)
  assert (cut['info'] == PA.BIT_TRUNCATED).all() and np.array_equal(cut['path_cells'], o24['path_cells'][:, :5]) and np.array_equal(cut['th_init'], o24['th_init'])
  assert np.array_equal(cut['num_cells'], o24['num_cells'])
  i = g24.names.index('goal_last_row_and_column')
  assert o24['path_cells'][i][o24['num_cells'][i] - 1] == 23 * 40 + 39
  # the ragged serpentine crosses both chunk boundaries of its 130 columns
  o100 = PC.expected('g100')[0]
  cols = o100['path_cells'][0][:o100['num_cells'][0]] % 130
  assert cols.min() < 64 and ((cols >= 64) & (cols < 128)).any() and cols.max() >= 128
  # fp32 tensors see a rounded grid and rounded points: the discrete results of these cases do not move
  for name in PC.GROUPS:
    a, b = PC.expected(name)[0], PC.expected(name, 'f32')[0]
    assert np.array_equal(a['info'], b['info']) and np.array_equal(a['field'], b['field']) and np.array_equal(a['path_cells'], b['path_cells']), name


@pytest.mark.parametrize('name', PC.PROPERTY_GROUPS)
def test_feasibility_property(name):
  """info == 0 => every state's bilinear distance exceeds the clearance: the polyline between cell points runs inside pixel squares whose four corners are free (an
  axis move along an edge between two free cells, a diagonal move only where the two other corners are free as well); the stubs at the ends run inside the pixel
  squares of the start and the goal, whose corners are free because the pair was sampled 0.1 above the clearance on cells of at most 0.07 (the field is
  1-Lipschitz: a corner lies within sqrt(2) * 0.07 < 0.1 of the point)."""
  g = PC.group(name)
  out, _, _ = PC.expected(name)
  assert (g.x_lims[1] - g.x_lims[0]) / g.W <= 0.07 and (out['info'] == 0).all() and out['num_cells'].min() >= 5
  worst = np.inf
  for b in range(len(g.names)):
    d = np.array([PO.signed_distance(g.sdfs[g.env[b]], x, y, g.x_lims, g.y_lims) for x, y in out['th_init'][b][:, :2]])
    assert (d > g.clearance).all(), (name, b, d.min())
    worst = min(worst, d.min())
    # and not only the n states: the polyline itself, sampled finely
    dense = PA.resample([tuple(g.start[b, 0, :2])] + [PA.point_of(int(v) // g.W, int(v) % g.W, g.W, g.x_lims, g.y_lims) for v in out['path_cells'][b][:out['num_cells'][b]]] +
                        [tuple(g.goal[b, 0, :2])], 40 * g.n, g.start[b, 0, :2], g.goal[b, 0, :2], g.t_sec)[0]
    assert min(PO.signed_distance(g.sdfs[g.env[b]], x, y, g.x_lims, g.y_lims) for x, y in dense[:, :2]) > g.clearance, (name, b)
  # the straight lines of the same pairs are NOT all feasible: the cases would show nothing otherwise
  hit = 0
  for b in range(len(g.names)):
    line = PO.straight_line(g.start[b, 0, :2], g.goal[b, 0, :2], g.n, g.t_sec)
    hit += min(PO.signed_distance(g.sdfs[g.env[b]], x, y, g.x_lims, g.y_lims) for x, y in line[:, :2]) <= g.clearance
  assert hit >= 1, name


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
  assert C.sizeof(_capi.DgpPathParams) == 8 + 2 * 4      # include/dgpmp2_hip.h: one double, two int32
  assert _capi.DgpPathParams.max_sweeps.offset == 8 and _capi.DgpPathParams.path_cap.offset == 12
  assert 'init_paths' in _capi.CApi.SYMBOLS and api.init_paths is not None and api.abi_version() == 7
  p = _capi.Solver.path_params(0.8)
  assert (p.clearance, p.max_sweeps, p.path_cap) == (0.8, 64, 0)


def test_init_paths_validates_arguments_without_gpu(api):
  s = _capi.Solver(_cfg())
  ok_sdf, ok = s.sdf_arg(0x1000, 16, 16, 0), s.path_params(0.8, 8, 4)
  call = lambda solver, sdf, p, batch=8, **kw: solver.init_paths(batch, sdf, p, 0x1000, 0x1000, 0x1000, 0x1000, **kw)

  def refused(*a, **kw):
    with pytest.raises(_capi.DgpError) as e:
      call(*a, **kw)
    assert len(str(e.value)) > 20
    return e.value
  s3 = _capi.Solver(_cfg(dof=3, Q_c_inv=[[1, 0, 0], [0, 1, 0], [0, 0, 1]]))
  e = refused(s3, ok_sdf, ok)
  assert e.code == _capi.DGP_EINVAL and 'dof' in str(e)
  assert refused(s, ok_sdf, None).code == _capi.DGP_EINVAL                                   # NULL params
  assert refused(s, None, ok).code == _capi.DGP_EINVAL                                       # NULL sdf
  assert refused(s, s.sdf_arg(None, 16, 16, 0), ok).code == _capi.DGP_EINVAL                 # ... or no grid in it
  e = refused(s, s.sdf_arg(0x1000, 16, 16, 0, layout=_capi.DGP_SDF_TILED4), ok)
  assert e.code == _capi.DGP_EINVAL and 'row-major' in str(e)                                # tiled grids are refused
  assert refused(s, s.sdf_arg(0x1000, 16, 16, 0, layout=7), ok).code == _capi.DGP_EINVAL
  for bad in (0, -1, 4097):
    e = refused(s, ok_sdf, s.path_params(0.8, bad, 4))
    assert e.code == _capi.DGP_EINVAL and 'max_sweeps' in str(e)
  e = refused(s, ok_sdf, s.path_params(0.8, 8, -1))
  assert e.code == _capi.DGP_EINVAL and 'path_cap' in str(e)
  e = refused(s, ok_sdf, s.path_params(float('nan'), 8, 4))
  assert e.code == _capi.DGP_EINVAL and 'NaN' in str(e)
  assert refused(s, s.sdf_arg(0x1000, 4097, 16, 0), ok).code == _capi.DGP_EINVAL             # H beyond 2^12
  assert refused(s, s.sdf_arg(0x1000, 16, 4097, 0), ok).code == _capi.DGP_EINVAL             # W beyond 2^12
  assert refused(s, s.sdf_arg(0x1000, 0, 16, 0), ok).code == _capi.DGP_EINVAL
  assert refused(s, ok_sdf, ok, batch=0).code == _capi.DGP_EINVAL and refused(s, ok_sdf, ok, batch=-2).code == _capi.DGP_EINVAL
  raw = lambda h, start=0x1000, goal=0x1000, th=0x1000, field=0x1000: api.init_paths(h, 8, C.byref(ok_sdf), None, C.byref(ok), start, goal, th, field, None, None, None, None, None)
  assert raw(None) == _capi.DGP_EINVAL and b'null handle' in api.last_error()
  for kw in (dict(start=None), dict(goal=None), dict(th=None), dict(field=None)):
    assert raw(s.handle, **kw) == _capi.DGP_EINVAL, kw
  # a request of dgp_time_next_launch does not survive a rejected call
  assert api.time_next_launch(0x10, 0x20) == _capi.DGP_OK
  assert raw(None) == _capi.DGP_EINVAL
  assert refused(s, ok_sdf, ok, batch=0).code == _capi.DGP_EINVAL      # (a surviving request would make no difference here: nothing is launched; the GPU test times a launch)
  assert api.time_next_launch(None, None) == _capi.DGP_OK


def test_front_end_refusals():
  import torch
  from dgpmp2_amd import datasets as D
  from dgpmp2_amd.datasets import problem_generation as PG
  assert D.init_paths is PG.init_paths and D.PathInfo is PG.PathInfo
  z = torch.zeros(1, 1, 4)
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    PG.init_paths(object(), torch.zeros(1, 1, 16, 16), z, z)
  with pytest.raises(ValueError, match='untile.*row-major'):      # a TiledSdf is refused, with the way out
    PG.init_paths(object(), _FakeCuda(1, 1, 4, 4, 4, 4), _FakeCuda(1, 1, 4), _FakeCuda(1, 1, 4))
  with pytest.raises(ValueError, match='init'):
    PG.generate_dataset('unused', 'train', _FakeCuda(2, 16, 16), None, 1, init='rrt_star')
  info = PG.PathInfo(torch.tensor([0, 1, 2, 4, 8, 16], dtype=torch.int32), None, None)
  assert info.fell_back.tolist() == [False, True, True, True, True, False]
  assert info.unreachable.tolist() == [False, False, False, True, False, False] and info.unconverged.tolist() == [False, False, False, False, True, False]


class _FakeCuda(object):
  """a tensor that says it lives on the device: the argument checks are all that read it here"""

  def __new__(cls, *shape):
    import torch

    class T(torch.Tensor):
      @property
      def is_cuda(self): return True
    return torch.zeros(*shape).as_subclass(T)
