"""dgp_init_paths measured (nothing here is asserted anywhere):
  * kernel time (dgp_time_next_launch events, _capi.KernelTimer; median and minimum of back-to-back launches behind a warm-up) at B = 4096 problems on 256 x 256
    grids, one grid per problem, `forest` and `passage` maps from generate_obstacle_maps, start / goal pairs from sample_problems, float64 grids;
  * the sweeps each problem used (median, maximum): the kernel does not report them, so the batch is run at max_sweeps = 1, 2, ... and a problem's count is one more
    than the number of caps at which it is still flagged unconverged;
  * next to it: the host loop of tests/paths_oracle.py (dijkstra_field + trace + resample, wall clock per problem, a few problems), and the reference's own budget
    for its RRT* initialiser, QUOTED from its source (init_planner.plan(start_conf, goal_conf, 4.0), generate_optimal_paths_gpmp2.py:156-159), not measured: OMPL is
    not part of this build;
  * what the feature is for: the fraction of environments generate_dataset keeps with init='straight' and with init='grid_path', `forest`, `multi_obs` and
    `mixed_clutter`, 64 environments x 4 problems of 128 x 128 at the same seed.
Prints one JSON line.   usage: python profiles/tools/init_paths_time.py"""
import json, os, shutil, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench
import paths_oracle as PA
from dgpmp2_amd import _capi
from dgpmp2_amd.datasets import generate_dataset, generate_obstacle_maps, init_paths, sample_problems
from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
from dgpmp2_amd.robot_models import PointRobot2D
from dgpmp2_amd.utils.sdf_utils import sdf_2d_batch

B, S, N_STATES = 4096, 256, 64
RADIUS, EPS = 0.4, 0.4


def planner_of(n):
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(EPS)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': 50, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(RADIUS), 1, n, use_cuda=True), batch_size=1, use_cuda=True)


def kernel_us(launch, reps=12):
  timer = _capi.KernelTimer(reps)
  bench.prewarm(lambda k: launch(), 0.3, 3)
  for _ in range(reps):
    timer.arm(); launch()
  torch.cuda.synchronize()
  t = np.asarray(timer.durations_ms()) * 1e3
  return float(np.median(t)), float(t.min())


planner = planner_of(N_STATES)
out = {'config': 'B=%d problems, one %dx%d float64 grid each, n=%d, clearance %.1f (radius + epsilon), max_sweeps 64' % (B, S, S, N_STATES, RADIUS + EPS),
       'reference_rrt_star_budget_s_per_problem': 4.0,
       'reference_rrt_star_budget_source': 'init_planner.plan(start_conf, goal_conf, 4.0), datasets/generate_optimal_paths_gpmp2.py:156-159 -- quoted, not measured'}
for dataset_type in ('forest', 'passage'):
  kw = {'obstacle_sep': 0.0} if dataset_type == 'forest' else {}      # (a padded forest overlaps, and then caps, in most maps of a large batch: profiles/r08_obstacle_maps.json)
  print(dataset_type, file=sys.stderr, flush=True)
  images, oinfo = generate_obstacle_maps(planner, dataset_type, B, S, seed=1, **kw)
  sdf = sdf_2d_batch(images, padlen=0, res=10.0 / S)
  if sdf.dim() == 3: sdf = sdf.unsqueeze(1)
  startb, goalb, line, sinfo = sample_problems(planner, sdf, seed=1)
  th, info = init_paths(planner, sdf, startb, goalb, return_field=True)
  torch.cuda.synchronize()
  flags = info.flags.cpu().numpy()
  med, mn = kernel_us(lambda: init_paths(planner, sdf, startb, goalb, return_field=True))
  print(' kernel_us', med, mn, file=sys.stderr, flush=True)
  caps = list(range(1, 17))
  unconv = np.stack([init_paths(planner, sdf, startb, goalb, max_sweeps=k)[1].unconverged.cpu().numpy() for k in caps])
  sweeps = 1 + unconv.sum(0)
  in_coll = lambda t: planner.trajectory_metrics(t, sdf, eps=0.0).in_collision.cpu().numpy()
  rec = {'kernel_us': round(med, 1), 'kernel_us_min': round(mn, 1), 'us_per_problem': round(med / B, 3), 'sweeps_median': float(np.median(sweeps)), 'sweeps_max': int(sweeps.max()),
         'sweeps_beyond_%d' % caps[-1]: int(unconv[-1].sum()), 'maps_flagged': int((oinfo.capped | oinfo.overlapping).sum()), 'pairs_capped': int(sinfo.capped.sum()),
         'fell_back': int((flags & 15 != 0).sum()), 'start_or_goal_cell_blocked': int((flags & 3 != 0).sum()), 'unreachable_only': int((flags & 15 == 4).sum()),
         'mean_cells': round(float(info.num_cells.double().mean()), 1), 'mean_length_over_straight': round(float((info.length / (goalb - startb)[:, 0, :2].norm(dim=1)).mean()), 4),
         'initial_trajectory_in_collision_straight': int(in_coll(line).sum()), 'initial_trajectory_in_collision_grid_path': int(in_coll(th).sum())}
  # the host loop, the oracle's way, on a few problems
  n_host = 4
  sdf_h, s_h, g_h = sdf[:n_host, 0].cpu().numpy(), startb[:n_host].cpu().numpy(), goalb[:n_host].cpu().numpy()
  t0 = time.perf_counter()
  for b in range(n_host):
    free = PA.free_cells(sdf_h[b], RADIUS + EPS)
    sc, gc = (PA.cell_of(p[b, 0, 0], p[b, 0, 1], S, S, (-5.0, 5.0), (-5.0, 5.0)) for p in (s_h, g_h))
    D = PA.dijkstra_field(free, gc)
    if free[sc] and int(D[sc]) != PA.INF:
      cells = PA.trace(D, free, sc)
      PA.resample([tuple(s_h[b, 0, :2])] + [PA.point_of(r, c, S, (-5.0, 5.0), (-5.0, 5.0)) for r, c in cells] + [tuple(g_h[b, 0, :2])], N_STATES, s_h[b, 0, :2], g_h[b, 0, :2], 10.0)
  per = (time.perf_counter() - t0) / n_host
  rec['host_oracle_ms_per_problem'] = round(per * 1e3, 1)
  rec['host_oracle_s_for_batch'] = round(per * B, 1)
  rec['reference_budget_s_for_batch'] = 4.0 * B
  out[dataset_type] = rec
  del images, sdf, th, info

# what the feature is for
E, P, S2 = 64, 4, 128
planner = planner_of(N_STATES)
tmp = tempfile.mkdtemp()
for dataset_type in ('forest', 'multi_obs', 'mixed_clutter'):
  rec = {}
  for init in ('straight', 'grid_path'):
    okw = {'obstacle_sep': 0.0} if dataset_type in ('forest', 'mixed_clutter') else {}
    r = generate_dataset(os.path.join(tmp, dataset_type + '_' + init), 'train', None, planner, P, seed=9, dataset_type=dataset_type, num_envs=E, im_size=S2, obstacle_params=okw, init=init)
    through = len(r['env_numbers'])
    print(' kept', dataset_type, init, r['num_envs'], file=sys.stderr, flush=True)
    rec[init] = {'environments': E, 'through_the_chain': through, 'kept': r['num_envs'], 'kept_fraction': round(r['num_envs'] / E, 4),
                 'kept_fraction_of_chain': round(r['num_envs'] / max(through, 1), 4), 'problems_in_collision': int(r['in_coll'].sum()) if through else 0}
    if init == 'grid_path' and through: rec[init]['fell_back'] = int(r['path_info'].fell_back.sum())
  out['kept_' + dataset_type] = rec
shutil.rmtree(tmp, ignore_errors=True)
print(json.dumps(out))
