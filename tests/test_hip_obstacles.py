"""dgp_obstacle_maps on the GPU, through the C-ABI and through the Python front end (dgpmp2_amd.datasets.obstacle_maps).

  * bit-exact agreement with tests/obstacles_oracle.py -- image, boxes, num_boxes, draws, info -- for the inputs of tests/obstacles_cases.py: E = 9 maps of 32 x 37 (a
    width no vector divides: every row starts at another offset from a 16-byte boundary, and the image itself starts 3 / 1 / 1 elements behind one) and E = 130 maps of
    64 x 64; every dataset type, the mixed type, 44 obstacles, wrapped boxes, with and without keep-out points, environment numbers above 2^32; uint8, float32 and float64
    images.  Nothing is tolerated: every decision is discrete.  The image lies inside a larger buffer whose other bytes must come back untouched, and every output is
    pre-filled: each of its elements must be written;
  * independence: environment e is the same bits alone, in the batch and at another position of a batch;
  * max_draws = 1 caps (every output written), and after an overlap every further obstacle takes its last candidate;
  * the chain generate_obstacle_maps -> sdf_2d_batch -> sample_problems: every start and goal is feasible in the SDF of its own generated map;
  * generate_dataset(images=None, ...) writes a directory PlanningDataset reads; capture in a HIP graph and replay."""
import numpy as np
import pytest
import torch

import obstacles_cases as OC
import obstacles_oracle as OO
import problems_oracle as PO
from dgpmp2_amd import _capi

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = {'u8': (torch.uint8, np.uint8, _capi.DGP_U8, 3), 'f32': (torch.float32, np.float32, _capi.DGP_F32, 1), 'f64': (torch.float64, np.float64, _capi.DGP_F64, 1)}      # ..., elements in front of the image


def _solver():
  return _capi.Solver(_capi.make_config(num_states=16, dof=2, io_dtype=_capi.DGP_F64, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1,
                                        sphere_radius=0.4, Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4))


def c_params(gens):
  return [_capi.Solver.obstacle_params(g.kind, g.n_lo, g.n_hi, g.w_min, g.w_max, g.h_min, g.h_max, g.start_x, g.start_y, g.end_x, g.end_y, g.patch_size_obs, g.patch_size,
                                       g.max_draws) for g in gens]


def run(gens, E, H, W, dtype='u8', seed=0, first_env=0, start=None, goal=None, optional=True, lead=None):
  """dgp_obstacle_maps through the ctypes binding -> (image (E,H,W), boxes, num_boxes, draws, info) as numpy arrays (None for the optional ones when not asked for)"""
  s = _solver()
  tt, nt, code, off = DTYPES[dtype]
  if lead is not None: off = lead
  fill = 7 if dtype == 'u8' else -77.0
  N, tail = E * H * W, 64
  buf = torch.full((off + N + tail,), fill, dtype=tt, device=DEV)
  image = buf[off:off + N]
  dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)
  sp, gp = dev(start), dev(goal)
  P = 0 if sp is None and gp is None else int((sp if sp is not None else gp).shape[1])
  boxes = torch.full((E, 64, 4), -7, dtype=torch.int32, device=DEV) if optional else None
  draws = torch.full((E, 64), -7, dtype=torch.int32, device=DEV) if optional else None
  num_boxes, info = (torch.full((E,), -7, dtype=torch.int32, device=DEV) if optional else None for _ in range(2))
  ptr = lambda t: None if t is None else t.data_ptr()
  s.obstacle_maps(E, H, W, c_params(gens), image.data_ptr(), code, seed=seed, first_env=first_env, start_pts=ptr(sp), goal_pts=ptr(gp), num_pts=P, boxes=ptr(boxes),
                  num_boxes=ptr(num_boxes), draws=ptr(draws), info=ptr(info), stream=torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  b = buf.cpu().numpy()
  assert (b[:off] == fill).all() and (b[off + N:] == fill).all(), 'bytes outside the image were written'
  host = lambda t: None if t is None else t.cpu().numpy()
  return b[off:off + N].reshape(E, H, W), host(boxes), host(num_boxes), host(draws), host(info)


def run_case(name, dtype='u8', **kw):
  gen, (E, H, W), seed, first_env, P = OC.CASES[name]
  start, goal = OC.points(name)
  return run(OC.gens_of(gen, 32 if H == 32 else 64), E, H, W, dtype, seed, first_env, start, goal, **kw)


def assert_equals_oracle(got, want, dtype, what):
  image, boxes, num_boxes, draws, info = got
  count, w_boxes, w_num, w_draws, w_info = want
  w_image = OO.image_of(count, DTYPES[dtype][1])
  for name, g, w in (('info', info, w_info), ('num_boxes', num_boxes, w_num), ('draws', draws, w_draws), ('boxes', boxes, w_boxes), ('image', image, w_image)):
    if g is None: continue
    assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
    bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
    assert bad.size == 0, '%s: %s differs from the oracle for %d environments, first %s: got %s want %s' % (
        what, name, bad.size, bad[:5], g[bad[0]].ravel()[:12], w[bad[0]].ravel()[:12])


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('name', sorted(OC.CASES))
def test_bit_exact_against_the_oracle(name, dtype):
  want = OC.expected(name)
  assert not (want[4] & 1).any()      # (tests/test_obstacles_oracle.py holds the inputs to this)
  assert_equals_oracle(run_case(name, dtype), want, dtype, '%s %s' % (name, dtype))


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_every_alignment_of_the_image(dtype):
  """the image 0 .. 16 bytes behind a 16-byte boundary: whole rows, heads and tails of every length"""
  name = 'small_multi_obs'
  want = OC.expected(name)
  esz = np.dtype(DTYPES[dtype][1]).itemsize
  for lead in range(0, 16 // esz + 1):
    assert_equals_oracle(run_case(name, dtype, lead=lead), want, dtype, '%s %s lead %d' % (name, dtype, lead))
  # ... and maps whose every row starts on a boundary (64 x 64 behind an aligned pointer): the launch then deals exactly one row of chunks to a lane group
  assert_equals_oracle(run_case('main_tar_pit', dtype, lead=0), OC.expected('main_tar_pit'), dtype, 'main_tar_pit %s aligned' % dtype)


def test_optional_outputs_may_be_null():
  name = 'small_passage'
  got = run_case(name, 'f32', optional=False)
  assert got[1] is None and got[4] is None
  assert_equals_oracle(got, OC.expected(name), 'f32', name + ' image only')


def _same(a, b):
  return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('name', ['small_forest', 'main_mixed'])
def test_independent_of_batch_size_and_position(name):
  gen, (E, H, W), seed, first_env, P = OC.CASES[name]
  gens = OC.gens_of(gen, 32 if H == 32 else 64)
  start, goal = OC.points(name)
  full = run(gens, E, H, W, 'u8', seed, first_env, start, goal)
  assert_equals_oracle(full, OC.expected(name), 'u8', name)
  assert _same(full, run(gens, E, H, W, 'u8', seed, first_env, start, goal)), 'two runs differ'
  h = E // 2 + 1      # the second part of a split batch: every environment at another position
  second = run(gens, E - h, H, W, 'u8', seed, first_env + h, start[h:], goal[h:])
  assert _same([a[h:] for a in full], second), 'second part of a split batch'
  for j in (0, 1, E // 2, E - 1):      # alone
    one = run(gens, 1, H, W, 'u8', seed, first_env + j, start[j:j + 1], goal[j:j + 1])
    assert _same([a[j:j + 1] for a in full], one), 'environment %d alone' % j
  other = run(gens, E, H, W, 'u8', seed + 1, first_env, start, goal)
  assert not np.array_equal(other[0], full[0]) and not np.array_equal(other[3], full[3])      # another seed: other maps


def test_max_draws_of_one_caps_with_every_output_written():
  E, H, W = OC.SMALL
  for kind in ('tar_pit', 'passage'):
    g = OC.gens_of(kind, 32)[0]
    gens = [OO.Gen(g.kind, g.n_lo, g.n_hi, g.w_min, g.w_max, g.h_min, g.h_max, g.start_x, g.start_y, g.end_x, g.end_y, g.patch_size, g.patch_size_obs, max_draws=1)]
    start, goal = OC.points('small_' + kind)
    want = OO.generate(gens, E, H, W, 21, 0, start, goal)
    assert (want[4] & 1).any() and (want[3][want[3] >= 0] == 0).all()      # the first candidate or the cap
    for dtype in sorted(DTYPES):
      assert_equals_oracle(run(gens, E, H, W, dtype, 21, 0, start, goal), want, dtype, 'max_draws = 1 %s %s' % (kind, dtype))


def test_after_an_overlap_every_obstacle_takes_its_last_candidate():
  """padded boxes that wrap let obstacles overlap; from then on the reference accepts nothing, and with a small max_draws the cap is cheap enough for the oracle to
  walk through: the kernel takes candidate max_draws - 1 without evaluating the others -- the same map"""
  E, H, W = OC.SMALL
  g = OC.gens_of('wrap', 32)[0]
  gens = [OO.Gen(g.kind, 6, 9, g.w_min, g.w_max, g.h_min, g.h_max, g.start_x, g.start_y, g.end_x, g.end_y, g.patch_size, g.patch_size_obs, max_draws=8)]
  for seed, pts in ((8, False), (13, True)):
    start, goal = OC.points('small_wrap') if pts else (None, None)
    want = OO.generate(gens, E, H, W, seed, 0, start, goal)
    assert ((want[4] & 3) == 3).any() and ((want[4] & 3) == 0).any(), want[4]
    for dtype in ('u8', 'f64'):      # (float images: cells covered twice are -1)
      got = run(gens, E, H, W, dtype, seed, 0, start, goal)
      assert_equals_oracle(got, want, dtype, 'overlap seed %d %s' % (seed, dtype))
    assert got[0].min() < 0.0


# ---- the Python front end ---------------------------------------------------------------------------------------------------------------------------------------

def _planner(n=16, max_iters=10):
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': max_iters, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), 1, n, use_cuda=True), batch_size=1, use_cuda=True)


def _oracle_gens(sets, max_draws=4096):
  return [OO.Gen(max_draws=max_draws, **p) for p in ([sets] if isinstance(sets, dict) else sets)]


@pytest.mark.parametrize('dataset_type', ['tar_pit', 'forest', 'multi_obs', 'passage', 'mixed_clutter'])
def test_front_end_equals_the_oracle(dataset_type):
  from dgpmp2_amd.datasets import generate_obstacle_maps, dataset_params, reference_separations, confs_to_pixels
  planner = _planner()
  E, S = 12, 64
  sgd, sep = reference_separations(dataset_type, 0.4, 0.4, (-5.0, 5.0), S)
  if dataset_type in ('forest', 'mixed_clutter'): sep = 0.0      # (see tests/obstacles_cases.py: a padded forest overlaps, and then caps, in some environment of any batch)
  kw = {} if dataset_type not in ('forest', 'mixed_clutter') else {'obstacle_sep': sep}
  rs = np.random.RandomState(77)
  confs = torch.from_numpy(rs.uniform(-3.5, 3.5, (E, 1, 2))).to(DEV)      # (far enough from the edges for no patch to wrap)
  start_pts, goal_pts = confs_to_pixels(confs, (-5.0, 5.0), (-5.0, 5.0), S), confs_to_pixels(-confs, (-5.0, 5.0), (-5.0, 5.0), S)
  images, info = generate_obstacle_maps(planner, dataset_type, E, S, seed=31, first_env=5, start_pts=start_pts, goal_pts=goal_pts, max_draws=512, **kw)
  assert images.shape == (E, 1, S, S) and images.dtype == torch.uint8 and images.is_cuda
  want = OO.generate(_oracle_gens(dataset_params(dataset_type, S, sgd, sep), 512), E, S, S, 31, 5, start_pts.cpu().numpy(), goal_pts.cpu().numpy())
  got = (images[:, 0].cpu().numpy(), info.boxes.cpu().numpy(), info.num_boxes.cpu().numpy(), info.draws.cpu().numpy(), info.flags.cpu().numpy())
  assert_equals_oracle(got, want, 'u8', 'front end ' + dataset_type)
  assert np.array_equal(info.capped.cpu().numpy(), (want[4] & 1) != 0) and np.array_equal(info.overlapping.cpu().numpy(), (want[4] & 2) != 0)
  assert np.array_equal(info.wrapped.cpu().numpy(), (want[4] & 4) != 0)
  f64, _ = generate_obstacle_maps(planner.plan_layer, dataset_type, E, S, seed=31, first_env=5, start_pts=start_pts, goal_pts=goal_pts, max_draws=512, dtype=torch.float64, **kw)
  assert f64.dtype == torch.float64 and np.array_equal(f64[:, 0].cpu().numpy(), OO.image_of(want[0], np.float64))
  # the keep-out points are free, with their patches
  im = got[0]
  for e in range(E):
    if want[4][e] & 1: continue
    for x, y in np.concatenate([start_pts[e].cpu().numpy(), goal_pts[e].cpu().numpy()]):
      assert im[e, int(np.ceil(y)) - 1:int(np.ceil(y)) + 1, int(np.ceil(x)) - 1:int(np.ceil(x)) + 1].all(), (e, x, y)
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    generate_obstacle_maps(planner, dataset_type, E, S, start_pts=start_pts.cpu())


def test_chain_maps_to_sdf_to_problems():
  """generate_obstacle_maps -> sdf_2d_batch -> sample_problems: every start and goal is feasible in the SDF of its own generated map"""
  from dgpmp2_amd.datasets import generate_obstacle_maps, sample_problems
  from dgpmp2_amd.utils.sdf_utils import sdf_2d_batch
  planner = _planner()
  E, S, P = 10, 64, 3
  for dataset_type in ('tar_pit', 'passage'):
    images, oinfo = generate_obstacle_maps(planner, dataset_type, E, S, seed=3)
    assert not oinfo.capped.any() and not oinfo.overlapping.any()
    sdf = sdf_2d_batch(images, padlen=0, res=10.0 / S)      # (E,1,H,W) float64, from the uint8 images as they are
    env_index = torch.arange(E, device=DEV, dtype=torch.int32).repeat_interleave(P)
    startb, goalb, thb, info = sample_problems(planner, sdf, env_index=env_index, seed=4)
    assert not info.capped.any()
    sdf_h, im_h = sdf[:, 0].cpu().numpy(), images[:, 0].cpu().numpy()
    assert 0 < (im_h == 0).sum() < im_h.size // 2
    clearance = 0.4 + 0.4 + 0.1
    for b, (s, g) in enumerate(zip(startb.cpu().numpy(), goalb.cpu().numpy())):
      e = b // P
      for x, y in (s[0, :2], g[0, :2]):
        assert PO.is_feasible(sdf_h[e], x, y, clearance), (dataset_type, b, x, y)
        assert im_h[e, min(int((5.0 - y) / (10.0 / S)), S - 1), min(int((x + 5.0) / (10.0 / S)), S - 1)] == 1      # ... and its own cell is free in its own image


def test_generate_dataset_from_a_seed(tmp_path):
  from dgpmp2_amd.datasets import PlanningDataset, generate_dataset
  n, S, P, E = 16, 64, 2, 6
  planner = _planner(n)
  root = str(tmp_path / 'ds')
  r = generate_dataset(root, 'train', None, planner, P, seed=5, dataset_type='multi_obs', num_envs=E, im_size=S, obstacle_params={'max_draws': 3}, max_draws=512)
  oi = r['obstacle_info']
  flagged = (oi.capped | oi.overlapping).cpu().numpy()
  assert flagged.any() and not flagged.all()      # max_draws = 3: some maps cap, and are dropped before anything else runs
  assert sorted(r['kept'] + list(r['dropped'])) == list(range(E)) and r['num_envs'] == len(r['kept']) >= 1
  for e in range(E):
    if flagged[e]: assert e in r['dropped'] and 'obstacle' in r['dropped'][e]
  assert r['env_numbers'] == [e for e in range(E) if not flagged[e]] and r['images'].shape == (len(r['env_numbers']), 1, S, S)
  assert r['start'].shape == (len(r['env_numbers']) * P, 1, 4)
  ds = PlanningDataset(root, 'train')
  assert len(ds) == len(r['kept']) * P and ds.meta_data['num_envs'] == len(r['kept']) and ds.meta_data['im_size'] == S
  images = r['images'][:, 0].cpu().numpy()
  for k, e in enumerate(r['kept']):
    smp = ds[k * P]
    assert smp['th_opt'].shape == (n, 4) and smp['sdf'].shape == (1, S, S)
    assert np.array_equal(smp['im'].numpy()[0], images[r['env_numbers'].index(e)].astype(np.float64))      # the stored image is the generated map
  # the maps are those of the seed: the same call of the generator gives them again
  from dgpmp2_amd.datasets import generate_obstacle_maps
  again, _ = generate_obstacle_maps(planner, 'multi_obs', E, S, seed=5, max_draws=3)
  assert torch.equal(again[torch.tensor(r['env_numbers'], device=DEV)], r['images'])


def test_capture_and_replay():
  from dgpmp2_amd.datasets import generate_obstacle_maps
  planner = _planner()
  E, S = 20, 64
  draw = lambda: generate_obstacle_maps(planner, 'tar_pit', E, S, seed=9)
  eager = draw()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    draw()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = draw()
  tensors = lambda o: (o[0], o[1].boxes, o[1].num_boxes, o[1].draws, o[1].flags)
  for t in tensors(out): t.fill_(3)      # the replay, not the capture, must produce the values
  graph.replay()
  torch.cuda.synchronize()
  for a, b in zip(tensors(out), tensors(eager)):
    assert torch.equal(a, b)
  assert (out[0] == 0).any() and (out[1].num_boxes >= 5).all()
