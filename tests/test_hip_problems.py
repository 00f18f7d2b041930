"""dgp_sample_problems on the GPU, through the C-ABI and through the Python front end (dgpmp2_amd.datasets.problem_generation).

  * bit-exact agreement with tests/problems_oracle.py -- start, goal, th_init, draws, info -- on batches of 131 problems (two wavefronts' worth of lanes and a ragged
    tail) whose environments are mixed inside every wavefront (tests/problems_cases.py: first-draw acceptance, accepted draws beyond a problem's 16 lanes, both caps, the
    near-tries rule, diagonals kept and replaced; the counts are asserted), for n in {3, 16, 101} on 16 x 16, 22 x 18 and 32 x 32 grids, fp64 and fp32 I/O, row-major and
    tiled grids, a shared grid and per-environment grids addressed through env_index.  Nothing is tolerated: the decisions are discrete and the operation order is
    pinned; for fp32 I/O the expected values are the oracle's fp64 results rounded once;
  * independence: problem j is the same bits in the full batch, alone at first_problem = j and in the second half of a split batch; two runs, tiled and row-major grids,
    env_index and one grid per problem agree bit for bit;
  * capture in a HIP graph and replay;
  * generate_dataset end to end: three environments (one fully blocked) x two problems -> a directory PlanningDataset reads."""
import os

import numpy as np
import pytest
import torch

import harness
import problems_cases as PCS
import problems_oracle as PO
from dgpmp2_amd import _capi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NP_IO = {'f64': np.float64, 'f32': np.float32}
T_IO = {'f64': torch.float64, 'f32': torch.float32}


def _cfg(n, io, x_lims=(-5, 5), y_lims=(-5, 5), t_sec=PCS.T_SEC):
  return _capi.make_config(num_states=n, dof=2, io_dtype=_capi.DGP_F64 if io == 'f64' else _capi.DGP_F32, total_time_sec=t_sec, x_lims=x_lims, y_lims=y_lims,
                           K_s=0.01, K_g=0.01, reg=0.1, sphere_radius=0.4, Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4)


def run(n, io, grids, B, env_index=None, diagonal=None, seed=0, first_problem=0, tiled=False, **cfg):
  """dgp_sample_problems through the ctypes binding -> (start, goal, th_init, draws, info) as numpy arrays; grids (E, H, W), E = 1: shared; cfg: _cfg's limits and horizon"""
  s = _capi.Solver(_cfg(n, io, **cfg))
  E, H, W = grids.shape
  g4 = np.ascontiguousarray(grids[:, None]).astype(NP_IO[io])
  if tiled:
    til = harness.tile_np(g4)
    gd = torch.from_numpy(til).to(DEV)
    arg = s.sdf_arg(gd.data_ptr(), H, W, 0 if E == 1 else til[0].size, layout=_capi.DGP_SDF_TILED4)
  else:
    gd = torch.from_numpy(g4).to(DEV)
    arg = s.sdf_arg(gd.data_ptr(), H, W, 0 if E == 1 else H * W)
  dev = lambda a: None if a is None else torch.from_numpy(np.array(a, dtype=np.int32)).to(DEV)
  ei, dg = dev(env_index), dev(diagonal)
  if ei is not None: assert int(ei.min()) >= 0 and int(ei.max()) < E
  elif E > 1: assert E == B
  # NaN / -7 fills: every element of every output must be written
  start, goal = torch.full((B, 1, 4), float('nan'), dtype=T_IO[io], device=DEV), torch.full((B, 1, 4), float('nan'), dtype=T_IO[io], device=DEV)
  th = torch.full((B, n, 4), float('nan'), dtype=T_IO[io], device=DEV)
  draws, info = torch.full((B, 2), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
  sp = s.sample_params(PCS.CLEARANCE, max_draws=PCS.MAX_DRAWS, corner_inset=PCS.INSET)
  ptr = lambda t: None if t is None else t.data_ptr()
  s.sample_problems(B, arg, sp, start.data_ptr(), goal.data_ptr(), th.data_ptr(), seed=seed, first_problem=first_problem, env_index=ptr(ei), diagonal=ptr(dg),
                    draws=draws.data_ptr(), info=info.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  return tuple(t.cpu().numpy() for t in (start, goal, th, draws, info))


def assert_equals_oracle(got, want, n, io, what, t_sec=PCS.T_SEC):
  start, goal, th, draws, info = got
  w_start, w_goal, w_draws, w_info = want
  w_th = PO.th_init_of(w_start, w_goal, n, t_sec)
  r = lambda a: a.astype(NP_IO[io])      # the oracle's fp64 result, rounded once
  for name, g, w in (('info', info, w_info), ('draws', draws, w_draws), ('start', start, r(w_start)), ('goal', goal, r(w_goal)), ('th_init', th, r(w_th))):
    assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
    bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
    assert bad.size == 0, '%s: %s differs from the oracle for %d problems, first %s: got %s want %s' % (what, name, bad.size, bad[:5], g[bad[0]].ravel()[:8], w[bad[0]].ravel()[:8])


@pytest.mark.parametrize('sharing', ['env_index', 'shared'])
@pytest.mark.parametrize('tiled', [False, True], ids=['rowmajor', 'tiled'])
@pytest.mark.parametrize('io', ['f64', 'f32'])
@pytest.mark.parametrize('n', sorted(PCS.SIZES))
def test_bit_exact_against_the_oracle(n, io, tiled, sharing):
  H, W = PCS.SIZES[n]
  B = PCS.B_MAIN
  if sharing == 'env_index':
    f, env, diag, want = PCS.mixed(H, W)
    c = PCS.branch_counts(env, diag, want[2], want[3])
    PCS.check_branches(c)      # every branch is in the batch (a later edit of the inputs cannot silently lose one)
    seed = 7
  else:
    f, env, diag, want = PCS.shared(H, W)
    assert ((want[3] & 8) != 0).sum() > 0 and (diag < 0).sum() > 0
    seed = 11
  got = run(n, io, f, B, env, diag, seed=seed, tiled=tiled)
  assert_equals_oracle(got, want, n, io, 'n %d %s %s %s' % (n, io, 'tiled' if tiled else 'rowmajor', sharing))


@pytest.mark.parametrize('sharing', ['env_index', 'shared'])
@pytest.mark.parametrize('tiled', [False, True], ids=['rowmajor', 'tiled'])
@pytest.mark.parametrize('io', ['f64', 'f32'])
def test_bit_exact_against_the_oracle_at_other_limits(io, tiled, sharing):
  """x_lims = (-3, 7), y_lims = (-6, 2), total_time_sec = 7 on 26 x 20 grids (problems_cases.fields_nd): the box's bounds lbx / lby / ubx / uby, the pixel origins of x and
  y, the four limit tests and the corners of the diagonals all differ from one another and from the default's; tests/test_config_constants.py holds that each limit, and
  an x / y swap, changes every problem of this batch.  Bit-exact like the default parametrisation above."""
  n, B = PCS.ND_N, PCS.B_MAIN
  if sharing == 'env_index':
    f, env, diag, want = PCS.mixed_nd()
    PCS.check_branches(PCS.branch_counts(env, diag, want[2], want[3]))
    seed = 7
  else:
    f, env, diag, want = PCS.shared_nd()
    assert ((want[3] & 8) != 0).sum() > 0 and (diag < 0).sum() > 0
    seed = 11
  got = run(n, io, f, B, env, diag, seed=seed, tiled=tiled, x_lims=PCS.ND_X, y_lims=PCS.ND_Y, t_sec=PCS.ND_T_SEC)
  assert_equals_oracle(got, want, n, io, 'other limits %s %s %s' % (io, 'tiled' if tiled else 'rowmajor', sharing), t_sec=PCS.ND_T_SEC)


def _same(a, b):
  return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_independent_of_batch_position_split_layout_and_run():
  n, io = 16, 'f64'
  H, W = PCS.SIZES[n]
  B = PCS.B_MAIN
  f, env, diag, want = PCS.mixed(H, W)
  full = run(n, io, f, B, env, diag, seed=7)
  assert_equals_oracle(full, want, n, io, 'full batch')
  assert _same(full, run(n, io, f, B, env, diag, seed=7)), 'two runs differ'
  assert _same(full, run(n, io, f, B, env, diag, seed=7, tiled=True)), 'tiled and row-major grids differ'
  assert _same(full, run(n, io, f[env], B, None, diag, seed=7)), 'one grid per problem and env_index differ'
  # the second half of a split batch
  h = B // 2 + 1
  second = run(n, io, f, B - h, env[h:], diag[h:], seed=7, first_problem=h)
  assert _same([a[h:] for a in full], second), 'second half of a split batch'
  # single problems, one of every environment kind and diagonal state (problem j alone in its wavefront: three idle lane groups)
  for j in (0, 1, 2, 3, 4, 5, 9, 29, 66, B - 1):
    one = run(n, io, f, 1, env[j:j + 1], diag[j:j + 1], seed=7, first_problem=j)
    assert _same([a[j:j + 1] for a in full], one), 'problem %d alone' % j
  # another seed is another set of problems; problem numbers beyond 2^32 reach the counter's high word
  other = run(n, io, f, B, env, diag, seed=8)
  assert not np.array_equal(other[0], full[0])
  big = 1 << 40
  hi = run(n, io, f, 8, env[:8], diag[:8], seed=7, first_problem=big)
  w = PO.sample_problems(f, PCS.params(), 8, 7, big, env[:8], diag[:8])
  assert_equals_oracle(hi, w, n, io, 'first_problem = 2^40')
  assert not np.array_equal(hi[0], full[0][:8])


def test_optional_outputs_may_be_null_and_max_draws_of_one():
  n, io = 3, 'f32'
  H, W = PCS.SIZES[n]
  f, env, diag, want = PCS.mixed(H, W)
  s = _capi.Solver(_cfg(n, io))
  B = 37
  gd = torch.from_numpy(f[:, None].astype(np.float32)).to(DEV)
  arg = s.sdf_arg(gd.data_ptr(), H, W, H * W)
  ei = torch.from_numpy(env[:B].copy()).to(DEV)
  start, goal, th = (torch.full(sh, float('nan'), dtype=torch.float32, device=DEV) for sh in ((B, 1, 4), (B, 1, 4), (B, n, 4)))
  sp = s.sample_params(PCS.CLEARANCE, max_draws=1, corner_inset=PCS.INSET)      # the first candidate or the cap
  s.sample_problems(B, arg, sp, start.data_ptr(), goal.data_ptr(), th.data_ptr(), seed=7, env_index=ei.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  P = PO.Params(PCS.CLEARANCE, max_draws=1, corner_inset=PCS.INSET, total_time_sec=PCS.T_SEC)
  w_start, w_goal, w_draws, w_info = PO.sample_problems(f, P, B, 7, 0, env[:B], None)
  assert (w_draws == 0).all() and (w_info & 3).any() and not (w_info & 3).all()
  assert np.array_equal(start.cpu().numpy(), w_start.astype(np.float32)) and np.array_equal(goal.cpu().numpy(), w_goal.astype(np.float32))
  assert np.array_equal(th.cpu().numpy(), PO.th_init_of(w_start, w_goal, n, PCS.T_SEC).astype(np.float32))


# ---- the Python front end ---------------------------------------------------------------------------------------------------------------------------------------

def _planner(n, max_iters=10, x_lims=(-5.0, 5.0), y_lims=(-5.0, 5.0), t_sec=PCS.T_SEC):
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': t_sec, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': max_iters, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': list(x_lims), 'y_lims': list(y_lims)}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), 1, n, use_cuda=True), batch_size=1, use_cuda=True)


def test_front_end_equals_the_oracle_and_takes_tiled_grids():
  from dgpmp2_amd.datasets.problem_generation import sample_problems
  from dgpmp2_amd.utils.sdf_utils import tile_sdf
  n = 16
  H, W = PCS.SIZES[n]
  planner = _planner(n)
  f, env, diag, want = PCS.mixed(H, W)
  sdfb = torch.from_numpy(f[:, None].copy()).to(DEV)
  ei, dg = torch.from_numpy(env.copy()).to(DEV), torch.from_numpy(diag.copy()).to(DEV)
  kw = dict(env_index=ei, seed=7, diagonal=dg, max_draws=PCS.MAX_DRAWS, corner_inset=PCS.INSET)      # clearance: the default 0.4 + 0.4 + 0.1 is PCS.CLEARANCE
  assert 0.4 + 0.4 + 0.1 == PCS.CLEARANCE
  startb, goalb, thb, info = sample_problems(planner, sdfb, **kw)
  assert startb.is_cuda and startb.dtype == torch.float64 and thb.shape == (PCS.B_MAIN, n, 4)
  got = tuple(t.cpu().numpy() for t in (startb, goalb, thb, info.draws, info.flags))
  assert_equals_oracle(got, want, n, 'f64', 'front end')
  assert np.array_equal(info.capped.cpu().numpy(), (want[3] & 3) != 0) and np.array_equal(info.near_tries.cpu().numpy(), (want[3] & 4) != 0)
  assert np.array_equal(info.diagonal_replaced.cpu().numpy(), (want[3] & 8) != 0)
  t_start, t_goal, t_th, t_info = sample_problems(planner.plan_layer, tile_sdf(sdfb), **kw)
  assert torch.equal(t_start, startb) and torch.equal(t_goal, goalb) and torch.equal(t_th, thb) and torch.equal(t_info.flags, info.flags)
  s32 = sample_problems(planner, sdfb.float(), **kw)
  assert s32[0].dtype == torch.float32 and torch.equal(s32[0], startb.float()) and torch.equal(s32[2], thb.float())
  with pytest.raises(ValueError, match='env_index'):
    sample_problems(planner, sdfb, env_index=ei + 1, seed=7)
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    sample_problems(planner, sdfb.cpu(), env_index=ei)


def test_front_end_at_other_limits():
  """sample_problems(planner, ...) on a planner built with x_lims = (-3, 7), y_lims = (-6, 2), total_time_sec = 7: limits and horizon reach the kernel from the planner's
  dictionaries, each in its own place"""
  from dgpmp2_amd.datasets.problem_generation import sample_problems
  n = PCS.ND_N
  planner = _planner(n, x_lims=PCS.ND_X, y_lims=PCS.ND_Y, t_sec=PCS.ND_T_SEC)
  f, env, diag, want = PCS.mixed_nd()
  sdfb = torch.from_numpy(f[:, None].copy()).to(DEV)
  ei, dg = torch.from_numpy(env.copy()).to(DEV), torch.from_numpy(diag.copy()).to(DEV)
  startb, goalb, thb, info = sample_problems(planner, sdfb, env_index=ei, seed=7, diagonal=dg, max_draws=PCS.MAX_DRAWS, corner_inset=PCS.INSET)
  got = tuple(t.cpu().numpy() for t in (startb, goalb, thb, info.draws, info.flags))
  assert_equals_oracle(got, want, n, 'f64', 'front end, other limits', t_sec=PCS.ND_T_SEC)


def test_capture_and_replay():
  from dgpmp2_amd.datasets.problem_generation import sample_problems
  n = 16
  H, W = PCS.SIZES[n]
  planner = _planner(n)
  f, env, diag, want = PCS.mixed(H, W)
  sdfb = torch.from_numpy(f[:, None].copy()).to(DEV)
  ei, dg = torch.from_numpy(env.copy()).to(DEV), torch.from_numpy(diag.copy()).to(DEV)
  draw = lambda: sample_problems(planner, sdfb, env_index=ei, seed=7, diagonal=dg, max_draws=PCS.MAX_DRAWS, corner_inset=PCS.INSET)
  eager = draw()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    draw()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = draw()
  for t in out[:3] + (out[3].flags, out[3].draws): t.fill_(-3)      # the replay, not the capture, must produce the values
  graph.replay()
  torch.cuda.synchronize()
  for a, b in zip(out[:3] + (out[3].flags, out[3].draws), eager[:3] + (eager[3].flags, eager[3].draws)):
    assert torch.equal(a, b)
  assert_equals_oracle(tuple(t.cpu().numpy() for t in out[:3] + (out[3].draws, out[3].flags)), want, n, 'f64', 'replayed graph')


def test_generate_dataset_end_to_end(tmp_path):
  from dgpmp2_amd.datasets import PlanningDataset
  from dgpmp2_amd.datasets.problem_generation import generate_dataset
  n, S = 16, 32
  planner = _planner(n)
  im = np.ones((3, S, S))
  im[0, 4:8, 14:18] = 0.0        # small obstacles off both diagonals
  im[1] = 0.0                     # fully blocked: no feasible point, dropped
  im[2, 14:18, 2:6] = 0.0
  im[2, 14:18, 26:30] = 0.0
  images = torch.from_numpy(im).to(DEV)
  root = str(tmp_path / 'ds')
  r = generate_dataset(root, 'train', images, planner, 2, seed=5, first_diagonal=True, corner_inset=1.0, max_draws=512)
  assert r['num_envs'] == 2 and r['kept'] == [0, 2] and list(r['dropped']) == [1] and 'max_draws' in r['dropped'][1]
  capped = r['info'].capped.cpu().numpy()
  assert capped[2:4].all() and not capped[[0, 1, 4, 5]].any()
  assert sorted(os.listdir(os.path.join(root, 'train', 'im_sdf'))) == ['0_im.png', '0_sdf.npy', '1_im.png', '1_sdf.npy']
  assert sorted(os.listdir(os.path.join(root, 'train', 'opt_trajs_gpmp2'))) == ['env_%d_prob_%d.npz' % (e, j) for e in (0, 1) for j in (0, 1)]
  ds = PlanningDataset(root, 'train')
  assert len(ds) == 4 and ds.meta_data['num_envs'] == 2 and ds.meta_data['probs_per_env'] == 2 and ds.meta_data['im_size'] == S
  start, goal, th_init, th_opt = (r[k].cpu().numpy() for k in ('start', 'goal', 'th_init', 'th_opt'))
  sdfs, ths = [], []
  for k, e in enumerate((0, 2)):
    for j in range(2):
      smp, b = ds[k * 2 + j], e * 2 + j
      assert smp['th_opt'].shape == (n, 4) and smp['sdf'].shape == (1, S, S)
      # what was stored is what the sampler returned and the planner made of it; the initial trajectory runs from the start to the goal
      assert np.array_equal(smp['start'].numpy(), start[b]) and np.array_equal(smp['goal'].numpy(), goal[b]) and np.array_equal(smp['th_opt'].numpy(), th_opt[b])
      assert np.allclose(th_init[b, 0, :2], start[b, 0, :2], rtol=0, atol=1e-14) and np.allclose(th_init[b, n - 1, :2], goal[b, 0, :2], rtol=0, atol=1e-14)
      assert np.array_equal(smp['im'].numpy()[0], im[e])
      sdfs.append(smp['sdf']); ths.append(smp['th_opt'])
  # every stored trajectory is collision-free by the metric the generation used
  m = planner.trajectory_metrics(torch.stack(ths).to(DEV), torch.stack(sdfs).to(DEV), eps=0.0)
  assert not m.in_collision.any() and not r['in_coll'].cpu().numpy()[[0, 1, 4, 5]].any()
  # the first problem of an environment is a diagonal (kept where both corners are free, replaced otherwise)
  draws, flags = r['info'].draws.cpu().numpy(), r['info'].flags.cpu().numpy()
  for b in (0, 4):
    assert (draws[b] == -1).all() or (flags[b] & 8)
  assert (draws[[1, 5]] >= 0).all()
