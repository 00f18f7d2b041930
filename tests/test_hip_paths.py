"""dgp_init_paths on the GPU, through the C-ABI and through the Python front end (dgpmp2_amd.datasets.problem_generation).

  * against tests/paths_oracle.py on every case of tests/paths_cases.py: field, path_cells, num_cells and info BIT FOR BIT (the decisions are discrete, the rule is
    pinned); th_init and length within the project's parity bounds, 1e-9 (fp64) / 1e-5 (fp32) absolute in a workspace of +-5 -- for fp32 tensors the oracle sees the
    grid and the points the kernel sees, rounded once on the way in.  Grids addressed through env_index, one grid per problem, and one shared grid;
  * batches of 1, 5 and 67: a problem is the same bits wherever it stands, and however the front end chunks the batch;
  * bit 3 (max_sweeps = 1 on the serpentine) and bit 4 (path_cap below L); every optional output NULL;
  * fallback rows equal dgp_sample_problems' straight lines bit for bit;
  * sample_problems(init='grid_path') and generate_dataset(init='grid_path') equal init_paths on their own pairs; the files are written;
  * capture in a HIP graph and replay; dgp_time_next_launch is consumed by the call's kernel."""
import math
import os

import numpy as np
import pytest
import torch

import paths_cases as PC
import paths_oracle as PA
import problems_oracle as PO
from dgpmp2_amd import _capi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NP_IO = {'f64': np.float64, 'f32': np.float32}
T_IO = {'f64': torch.float64, 'f32': torch.float32}
TOL = {'f64': 1e-9, 'f32': 1e-5}      # the project's parity bounds, absolute (coordinates within +-5)


def _cfg(g, io):
  return _capi.make_config(num_states=g.n, dof=2, io_dtype=_capi.DGP_F64 if io == 'f64' else _capi.DGP_F32, total_time_sec=g.t_sec, x_lims=g.x_lims, y_lims=g.y_lims,
                           K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4, Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4)


def run(g, io, max_sweeps, path_cap, sel=None, grids='env_index', optional=True, timer=None):
  """dgp_init_paths through the ctypes binding for the problems `sel` (indices into the group, default all) -> dict of numpy arrays.
  grids: 'env_index' (the group's maps and an index per problem), 'per_sample' (one grid per problem), 'shared' (every selected problem lives in one map)."""
  sel = np.arange(len(g.names)) if sel is None else np.asarray(sel)
  B = len(sel)
  s = _capi.Solver(_cfg(g, io))
  env = g.env[sel]
  if grids == 'env_index': maps, ei, stride = g.sdfs, torch.from_numpy(env.copy()).to(DEV), g.H * g.W
  elif grids == 'per_sample': maps, ei, stride = g.sdfs[env], None, g.H * g.W
  else:
    assert len(set(env.tolist())) == 1
    maps, ei, stride = g.sdfs[env[:1]], None, 0
  gd = torch.from_numpy(np.ascontiguousarray(maps).astype(NP_IO[io])).to(DEV)
  start, goal = (torch.from_numpy(a[sel].astype(NP_IO[io])).to(DEV) for a in (g.start, g.goal))
  # NaN / -7 fills: every element of every output must be written
  th = torch.full((B, g.n, 4), float('nan'), dtype=T_IO[io], device=DEV)
  field = torch.full((B, g.H, g.W), -7, dtype=torch.int32, device=DEV)
  cells = torch.full((B, path_cap), -7, dtype=torch.int32, device=DEV)
  num, info = (torch.full((B,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
  length = torch.full((B,), float('nan'), dtype=torch.float64, device=DEV)
  opt = (lambda t: t.data_ptr()) if optional else (lambda t: None)
  if timer is not None: timer.arm()
  s.init_paths(B, s.sdf_arg(gd.data_ptr(), g.H, g.W, stride), s.path_params(g.clearance, max_sweeps, path_cap), start.data_ptr(), goal.data_ptr(), th.data_ptr(),
               field.data_ptr(), env_index=None if ei is None else ei.data_ptr(), path_cells=opt(cells) if path_cap else None, num_cells=opt(num), length=opt(length),
               info=opt(info), stream=torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  return dict(th_init=th.cpu().numpy(), field=field.cpu().numpy().view(np.uint32), path_cells=cells.cpu().numpy(), num_cells=num.cpu().numpy(), length=length.cpu().numpy(),
              info=info.cpu().numpy())


def assert_equals_oracle(got, want, io, what, sel=None):
  pick = (lambda a: a) if sel is None else (lambda a: a[np.asarray(sel)])
  for name in ('info', 'num_cells', 'path_cells', 'field'):
    w, g_ = pick(want[name]), got[name]
    assert g_.dtype == w.dtype and g_.shape == w.shape, (what, name, g_.dtype, w.dtype, g_.shape, w.shape)
    bad = np.flatnonzero((g_ != w).reshape(len(w), -1).any(1))
    assert bad.size == 0, '%s: %s differs from the oracle for problems %s: got %s want %s' % (what, name, bad[:5], g_[bad[0]].ravel()[:12], w[bad[0]].ravel()[:12])
  e_th, e_len = np.abs(got['th_init'].astype(np.float64) - pick(want['th_init'])).max(), np.abs(got['length'] - pick(want['length'])).max()
  print('%s: max |th_init - oracle| = %.3e, max |length - oracle| = %.3e' % (what, e_th, e_len))
  assert np.isfinite(got['th_init']).all() and e_th <= TOL[io], (what, e_th)
  assert e_len <= TOL['f64' if io == 'f64' else 'f32'], (what, e_len)


@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('name', PC.GROUPS)
def test_equals_the_oracle(name, io):
  g = PC.group(name)
  want, ms, cap = PC.expected(name, io)
  got = run(g, io, ms, cap)
  assert_equals_oracle(got, want, io, '%s %s env_index' % (name, io))
  if io == 'f64':      # computed in fp64 and rounded once on store: with fp64 tensors the trajectory is the oracle's to the last few ulps of a coordinate
    assert np.abs(got['th_init'] - want['th_init']).max() <= 1e-13, name


@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_grid_modes(io):
  """one grid per problem and a shared grid give the bits of env_index"""
  for name in ('g16', 'g24'):
    g = PC.group(name)
    want, ms, cap = PC.expected(name, io)
    base = run(g, io, ms, cap)
    per = run(g, io, ms, cap, grids='per_sample')
    assert_equals_oracle(per, want, io, '%s %s per_sample' % (name, io))
    assert all(base[k].tobytes() == per[k].tobytes() for k in base), name
    sel = np.flatnonzero(g.env == 0)
    sh = run(g, io, ms, cap, sel=sel, grids='shared')
    assert_equals_oracle(sh, want, io, '%s %s shared' % (name, io), sel)
    assert all(base[k][sel].tobytes() == sh[k].tobytes() for k in base), name


def test_batch_sizes_and_positions():
  """B = 1, 5, 67: the same problem gives the same bits alone, in a short batch and at every position of a batch longer than one launch wave"""
  g = PC.group('g16')
  want, ms, cap = PC.expected('g16')
  P = len(g.names)
  sel67 = (np.arange(67) * 4) % P      # every problem at several positions
  big = run(g, 'f64', ms, cap, sel=sel67)
  assert_equals_oracle(big, want, 'f64', 'B = 67', sel67)
  sel5 = np.array([7, 0, 4, 5, 2])
  five = run(g, 'f64', ms, cap, sel=sel5)
  assert_equals_oracle(five, want, 'f64', 'B = 5', sel5)
  for j in range(P):
    one = run(g, 'f64', ms, cap, sel=[j])
    for k in one:
      assert one[k][0].tobytes() == big[k][np.flatnonzero(sel67 == j)[0]].tobytes(), (j, k)
      for pos in np.flatnonzero(sel67 == j): assert big[k][pos].tobytes() == one[k][0].tobytes(), (j, k, pos)
  for pos, j in enumerate(sel5):
    for k in five: assert five[k][pos].tobytes() == big[k][np.flatnonzero(sel67 == j)[0]].tobytes(), (j, k)


def test_unconverged_truncated_and_null_outputs():
  g = PC.group('g64')
  one, _, _ = PC.expected('g64', 'f64', 1, 240)
  got = run(g, 'f64', 1, 240)
  assert_equals_oracle(got, one, 'f64', 'max_sweeps = 1')
  assert (got['info'] & PA.BIT_UNCONVERGED).any()
  g = PC.group('g24')
  cut, _, _ = PC.expected('g24', 'f64', 5, 5)
  got = run(g, 'f64', 5, 5)
  assert_equals_oracle(got, cut, 'f64', 'path_cap = 5')
  assert (got['info'] == PA.BIT_TRUNCATED).all()
  # every optional output NULL, no path_cells at all: th_init and field are the same bits
  want, ms, cap = PC.expected('g24')
  full, bare = run(g, 'f64', ms, cap), run(g, 'f64', ms, 0, optional=False)
  assert bare['th_init'].tobytes() == full['th_init'].tobytes() and bare['field'].tobytes() == full['field'].tobytes()
  assert (bare['num_cells'] == -7).all() and (bare['info'] == -7).all()      # (untouched)


def _planner(n, x_lims=(-5.0, 5.0), y_lims=(-5.0, 5.0), t_sec=10.0, max_iters=10, radius=0.4, eps=0.4):
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(eps)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': t_sec, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': max_iters, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': list(x_lims), 'y_lims': list(y_lims)}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(radius), 1, n, use_cuda=True), batch_size=1, use_cuda=True)


def _front_end_call(g, io='f64', **kw):
  """the planner and the device tensors of a group, made once -> a function that calls init_paths on them"""
  from dgpmp2_amd.datasets.problem_generation import init_paths
  planner = _planner(g.n, g.x_lims, g.y_lims, g.t_sec)
  sdfb = torch.from_numpy(g.sdfs[:, None].astype(NP_IO[io])).to(DEV)
  ei = torch.from_numpy(g.env.copy()).to(DEV)
  start, goal = (torch.from_numpy(a.astype(NP_IO[io])).to(DEV) for a in (g.start, g.goal))
  return lambda: init_paths(planner, sdfb, start, goal, env_index=ei, clearance=g.clearance, **kw)


def _front_end(g, io='f64', **kw):
  return _front_end_call(g, io, **kw)()


def _as_dict(th, info):
  torch.cuda.synchronize()
  d = dict(th_init=th.cpu().numpy(), num_cells=info.num_cells.cpu().numpy(), length=info.length.cpu().numpy(), info=info.flags.cpu().numpy())
  if info.path_cells is not None: d['path_cells'] = info.path_cells.cpu().numpy()
  if info.field is not None: d['field'] = info.field.cpu().numpy().view(np.uint32)
  return d


def test_front_end_and_chunking(monkeypatch):
  from dgpmp2_amd.datasets import problem_generation as PG
  g = PC.group('g16')
  want, ms, cap = PC.expected('g16')
  th, info = _front_end(g, max_sweeps=ms, path_cap=cap, return_field=True)
  assert th.is_cuda and th.dtype == torch.float64 and info.field.shape == (len(g.names), 16, 16)
  whole = _as_dict(th, info)
  assert_equals_oracle(whole, want, 'f64', 'front end')
  assert np.array_equal(info.fell_back.cpu().numpy(), (want['info'] & 15) != 0) and np.array_equal(info.unreachable.cpu().numpy(), (want['info'] & 4) != 0)
  assert not info.unconverged.any()
  # chunks of two problems (the scratch bound lowered to two 16 x 16 fields): the same bits, no field returned
  monkeypatch.setattr(PG, '_FIELD_SCRATCH_BYTES', 2 * 16 * 16 * 4)
  th_c, info_c = _front_end(g, max_sweeps=ms, path_cap=cap)
  chunked = _as_dict(th_c, info_c)
  assert info_c.field is None and all(chunked[k].tobytes() == whole[k].tobytes() for k in chunked)
  th_n, info_n = _front_end(g, max_sweeps=ms)      # path_cap 0: no path_cells, bit 4 wherever a path was traced
  assert info_n.path_cells is None and torch.equal(th_n, th) and np.array_equal(info_n.flags.cpu().numpy() & 15, want['info'] & 15)
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    PG.init_paths(_planner(g.n), torch.zeros(1, 1, 16, 16), th[:, :1], th[:, :1])
  from dgpmp2_amd.utils.sdf_utils import tile_sdf
  with pytest.raises(ValueError, match='untile'):
    PG.init_paths(_planner(g.n), tile_sdf(torch.zeros(1, 1, 16, 16, dtype=torch.float64, device=DEV)), th[:1, :1], th[:1, :1])


def test_fallback_rows_equal_the_samplers_straight_lines_and_grid_path_switch():
  """pairs sampled by dgp_sample_problems; at a clearance nothing satisfies, every problem falls back: th_init must be the sampler's straight lines bit for bit.
  (fp64 tensors.  With fp32 tensors the sampler draws its line between the fp64 points it sampled and init_paths between the fp32 points it is given, so the two can
  differ in the last bit: there the rows are held, bit for bit, against the sampler's formula -- problems_oracle.straight_line -- on the fp32 points, rounded once.)
  At the planner's own clearance sample_problems(init='grid_path') returns what init_paths returns for those pairs."""
  from dgpmp2_amd.datasets.problem_generation import init_paths, sample_problems
  g = PC.group('p64')
  planner = _planner(g.n, g.x_lims, g.y_lims, g.t_sec, radius=0.1, eps=0.1)      # default clearances: 0.2 for the path, 0.3 for the sampler -- the group's
  for io in ('f64', 'f32'):
    sdfb = torch.from_numpy(g.sdfs[:, None].astype(NP_IO[io])).to(DEV)
    startb, goalb, line, sinfo = sample_problems(planner, sdfb, num_problems=37, seed=3)
    assert not sinfo.capped.any()
    th, info = init_paths(planner, sdfb, startb, goalb, clearance=50.0)
    assert info.fell_back.all() and (info.num_cells == 0).all()
    if io == 'f64': assert torch.equal(th, line)
    rounded = PO.th_init_of(startb.cpu().numpy().astype(np.float64), goalb.cpu().numpy().astype(np.float64), g.n, g.t_sec).astype(NP_IO[io])
    assert np.array_equal(th.cpu().numpy(), rounded), io
    d = (goalb.double() - startb.double())[:, 0, :2].cpu().numpy()
    assert np.abs(info.length.cpu().numpy() - np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])).max() <= 1e-12
    s2, g2, th2, _ = sample_problems(planner, sdfb, num_problems=37, seed=3, init='grid_path')
    th3, info3 = init_paths(planner, sdfb, startb, goalb)
    assert torch.equal(s2, startb) and torch.equal(g2, goalb) and torch.equal(th2, th3) and not info3.fell_back.any()
    assert not torch.equal(th3, line) and torch.equal(th3[:, 0, :2], startb[:, 0, :2]) and torch.equal(th3[:, -1, :2], goalb[:, 0, :2])
    # the feasibility property on the device's own result: every state clears the obstacles by more than the clearance (trajectory_metrics' hinge at eps = 0.1)
    if io == 'f64':
      m = planner.trajectory_metrics(th3, sdfb.expand(37, 1, g.H, g.W), eps=0.1)
      assert not m.in_collision.any()


def test_generate_dataset_with_grid_paths(tmp_path):
  from dgpmp2_amd.datasets import PlanningDataset
  from dgpmp2_amd.datasets.problem_generation import generate_dataset, init_paths
  from dgpmp2_amd.utils.sdf_utils import sdf_2d_batch
  n, S = 16, 64
  planner = _planner(n, (-2.0, 2.0), (-2.0, 2.0), radius=0.1, eps=0.1)
  im = np.ones((4, S, S))
  im[0, 24:40, 28:36] = 0.0            # a block in the middle
  im[1, :44, 30:34] = 0.0              # a wall from the top
  im[2, 20:, 30:34] = 0.0              # a wall from the bottom
  im[3, 10:20, 10:54] = 0.0; im[3, 44:54, 10:54] = 0.0      # two bars
  images = torch.from_numpy(im).to(DEV)
  root = str(tmp_path / 'ds')
  r = generate_dataset(root, 'train', images, planner, 2, seed=5, first_diagonal=False, require_collision_free=False, init='grid_path', max_draws=512)
  assert r['num_envs'] == 4 and r['kept'] == [0, 1, 2, 3] and not r['dropped']
  assert sorted(os.listdir(os.path.join(root, 'train', 'opt_trajs_gpmp2'))) == ['env_%d_prob_%d.npz' % (e, j) for e in range(4) for j in (0, 1)]
  assert len(PlanningDataset(root, 'train')) == 8
  sdf = sdf_2d_batch(images, padlen=0, res=4.0 / S).unsqueeze(1)
  ei = torch.arange(4, device=DEV, dtype=torch.int32).repeat_interleave(2)
  th, info = init_paths(planner, sdf, r['start'], r['goal'], env_index=ei)
  assert torch.equal(r['th_init'], th) and torch.equal(r['path_info'].flags, info.flags) and torch.equal(r['path_info'].length, info.length)
  assert not info.fell_back.any() and (info.num_cells > 0).all()
  plain = generate_dataset(str(tmp_path / 'plain'), 'train', images, planner, 2, seed=5, first_diagonal=False, require_collision_free=False, max_draws=512)
  assert plain['path_info'] is None and torch.equal(plain['start'], r['start']) and not torch.equal(plain['th_init'], r['th_init'])


def test_capture_and_replay():
  g = PC.group('g24')
  want, ms, cap = PC.expected('g24')
  call = _front_end_call(g, max_sweeps=ms, path_cap=cap, return_field=True)
  eager = _as_dict(*call())
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    call()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    th, info = call()
  for t in (th, info.flags, info.num_cells, info.length, info.path_cells, info.field): t.fill_(-3)      # the replay, not the capture, must produce the values
  graph.replay()
  replayed = _as_dict(th, info)
  assert all(replayed[k].tobytes() == eager[k].tobytes() for k in eager)
  assert_equals_oracle(replayed, want, 'f64', 'replayed graph')


def test_timed_launch_is_consumed_by_the_call():
  g = PC.group('g24')
  want, ms, cap = PC.expected('g24')
  timer = _capi.KernelTimer(1)
  plain = run(g, 'f64', ms, cap)
  timed = run(g, 'f64', ms, cap, timer=timer)
  t = timer.durations_ms()[0]
  print('dgp_init_paths, 4 problems on 24 x 40: %.4f ms' % t)
  assert math.isfinite(t) and t > 0.0 and all(plain[k].tobytes() == timed[k].tobytes() for k in plain)
  again = run(g, 'f64', ms, cap)
  assert all(plain[k].tobytes() == again[k].tobytes() for k in plain) and timer.durations_ms()[0] == t      # the request did not outlive the call it was armed for
