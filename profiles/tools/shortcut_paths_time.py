"""dgp_shortcut_paths measured (nothing here is asserted anywhere), on the inputs of profiles/r09_init_paths.json (profiles/tools/init_paths_time.py): B = 4096
problems on 256 x 256 grids, one grid per problem, `forest` and `passage` maps from generate_obstacle_maps, start / goal pairs from sample_problems, float64 grids,
n = 64, clearance radius + epsilon, check_step a quarter of a cell, no bound on the lookahead:
  * kernel time (dgp_time_next_launch events, _capi.KernelTimer; median and minimum of back-to-back launches behind a warm-up) of dgp_shortcut_paths NEXT TO
    dgp_init_paths on the same inputs, alternating;
  * vertices before (L + 2) and after, the length ratio new / grid path, both as means over the simplified problems, the share of problems with bit 3 set (a kept
    segment that is not visible), problems not simplified (fallbacks of dgp_init_paths), paths beyond path_cap;
  * what the step is for: initial trajectories in collision (trajectory_metrics, eps = 0) for the grid path and the shortcut path.
Prints one JSON line.   usage: python profiles/tools/shortcut_paths_time.py > profiles/r13_shortcut_paths.json"""
import json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.datasets import generate_obstacle_maps, init_paths, sample_problems, shortcut_paths
from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
from dgpmp2_amd.robot_models import PointRobot2D
from dgpmp2_amd.utils.sdf_utils import sdf_2d_batch

B, S, N_STATES = 4096, 256, 64
RADIUS, EPS = 0.4, 0.4
PATH_CAP = 4 * (S + S)
REPS = 12


def planner_of(n):
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(EPS)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': 50, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(RADIUS), 1, n, use_cuda=True), batch_size=1, use_cuda=True)


def kernel_us_alternating(launches, reps=REPS):
  """launches: {name: callable whose FIRST kernel is the one to time} -> {name: (median us, minimum us)}; the launches alternate inside one timed window"""
  timers = {k: _capi.KernelTimer(reps) for k in launches}
  bench.prewarm(lambda k: [f() for f in launches.values()], 0.3, 3)
  for _ in range(reps):
    for k, f in launches.items():
      timers[k].arm(); f()
  torch.cuda.synchronize()
  out = {}
  for k in launches:
    t = np.asarray(timers[k].durations_ms()) * 1e3
    out[k] = (float(np.median(t)), float(t.min()))
  return out


planner = planner_of(N_STATES)
layer = planner.plan_layer
out = {'config': 'B=%d problems, one %dx%d float64 grid each, n=%d, clearance %.1f (radius + epsilon), check_step res/4, lookahead unbounded, path_cap %d; inputs of r09_init_paths.json'
                 % (B, S, S, N_STATES, RADIUS + EPS, PATH_CAP)}
for dataset_type in ('forest', 'passage'):
  kw = {'obstacle_sep': 0.0} if dataset_type == 'forest' else {}
  print(dataset_type, file=sys.stderr, flush=True)
  images, oinfo = generate_obstacle_maps(planner, dataset_type, B, S, seed=1, **kw)
  sdf = sdf_2d_batch(images, padlen=0, res=10.0 / S)
  if sdf.dim() == 3: sdf = sdf.unsqueeze(1)
  startb, goalb, line, sinfo = sample_problems(planner, sdf, seed=1)
  th_grid, pinfo = init_paths(planner, sdf, startb, goalb, path_cap=PATH_CAP, return_field=True)
  th_sc, sc = shortcut_paths(planner, sdf, startb, goalb, th_grid, pinfo, vertex_cap=64)
  torch.cuda.synchronize()
  # the timed shortcut launch goes through the layer on a scratch trajectory (the front end's clone would be the first kernel of the call)
  sp = _capi.Solver.shortcut_params(RADIUS + EPS, 10.0 / S / 4, PATH_CAP, 0)
  pp = _capi.Solver.path_params(RADIUS + EPS, 64, PATH_CAP)
  scratch, cells, num = th_grid.clone(), pinfo.path_cells.contiguous(), pinfo.num_cells.contiguous()
  field = pinfo.field
  t = kernel_us_alternating({'init_paths': lambda: layer.init_paths(sdf, startb, goalb, pp, torch.float64, None, field),
                             'shortcut_paths': lambda: layer.shortcut_paths(sdf, startb, goalb, scratch, cells, num, sp, torch.float64)})
  print(' kernel_us', t, file=sys.stderr, flush=True)
  assert torch.equal(scratch, th_sc)      # (rewriting a simplified trajectory gives the same trajectory: rows of other problems are never touched)
  flags = sc.flags.cpu().numpy()
  simp = sc.simplified.cpu().numpy()
  before, after = (pinfo.num_cells.cpu().numpy() + 2)[simp], sc.num_vertices.cpu().numpy()[simp]
  ratio = (sc.length.cpu().numpy() / pinfo.length.cpu().numpy())[simp]
  in_coll = lambda th: planner.trajectory_metrics(th, sdf, eps=0.0).in_collision.cpu().numpy()
  out[dataset_type] = {
      'init_paths_kernel_us': round(t['init_paths'][0], 1), 'init_paths_kernel_us_min': round(t['init_paths'][1], 1),
      'shortcut_paths_kernel_us': round(t['shortcut_paths'][0], 1), 'shortcut_paths_kernel_us_min': round(t['shortcut_paths'][1], 1),
      'shortcut_us_per_problem': round(t['shortcut_paths'][0] / B, 3), 'shortcut_over_init_paths': round(t['shortcut_paths'][0] / t['init_paths'][0], 4),
      'problems_simplified': int(simp.sum()), 'not_simplified_fallback': int((flags & 1 != 0).sum()), 'input_truncated': int((flags & 2 != 0).sum()),
      'mean_vertices_before': round(float(before.mean()), 1), 'mean_vertices_after': round(float(after.mean()), 2), 'max_vertices_after': int(after.max()),
      'mean_length_ratio': round(float(ratio.mean()), 4), 'min_length_ratio': round(float(ratio.min()), 4), 'max_length_ratio': float(ratio.max()),
      'share_bit3_unverified': round(float((flags & 8 != 0).mean()), 4),
      'initial_trajectory_in_collision_grid_path': int(in_coll(th_grid).sum()), 'initial_trajectory_in_collision_shortcut_path': int(in_coll(th_sc).sum())}
  del images, sdf, th_grid, th_sc, pinfo, sc, scratch, field
print(json.dumps(out))
