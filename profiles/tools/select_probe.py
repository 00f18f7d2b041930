"""Time of the multi-start selection (dgp_select_samples) at B = 4096 problems, S = 8 samples, n = 64, K = 7, fp32 and fp64 I/O, on a shared 256 x 256 grid and on
one 256 x 256 grid per problem, warmed and back to back on the same device, next to what it replaces:
  * the kernel: dgp_time_next_launch events (_capi.KernelTimer), every output asked for -- and with best and status alone (no gather, no second barrier); the share of the HBM roof from the algorithmic bytes (B S n d read, B n d
    written, score / exclude and the outputs);
  * the dense check of the old recipe: dgp_gp_interpolate with the summary only -- one launch over the B S rows on the shared grid; on per-problem grids, where one
    launch would need an S-fold copy of the grids, S launches of B rows over the sample-major trajectories, between two HIP events;
  * the torch selection ops of the old recipe (where, full_like, argmin, arange, an advanced-index gather, any) between two HIP events;
  * plan_multistart end to end against the old recipe (sample_prior, forward() on the B S rows, interpolate, the torch ops) on the shared grid, wall clock around a
    device synchronisation: the recipe copies every per-sample result to the host, plan_multistart copies nothing.
Writes profiles/r16_select_samples.json and prints it.
usage: python profiles/tools/select_probe.py [output.json]"""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
from dgpmp2_amd.robot_models import PointRobot2D
from dgpmp2_amd.utils.sdf_utils import circles_sdf

dev = torch.device('cuda:0')
B, S, N, K, G = 4096, 8, 64, 7, 256
CIRCLES = ((-2.0, -1.0, 1.0), (1.5, 2.0, 0.8), (0.0, 0.0, 0.7), (2.5, -2.5, 0.9))


def quartiles(t):
  t = np.asarray(t, np.float64)
  return {'median': round(float(np.median(t)), 2), 'q1': round(float(np.percentile(t, 25)), 2), 'q3': round(float(np.percentile(t, 75)), 2), 'min': round(float(t.min()), 2)}


def planner():
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': N - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'plan_time': float('inf'), 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  env = {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}
  return DiffGPMP2Planner(gp, ob, pp, op, env, PointRobot2D(t(0.4), B * S, N, use_cuda=True), batch_size=B * S, use_cuda=True)


def events_us(fn, calls, reps):
  out = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls): fn()
    b.record(); torch.cuda.synchronize()
    out.append(a.elapsed_time(b) * 1e3 / calls)
  return out


def torch_selection(th, in_coll, err):
  """the old recipe's step 5 on (B,S) tensors: the collision-free sample with the smallest final error"""
  masked = torch.where(in_coll, torch.full_like(err, float('inf')), err)
  best = masked.argmin(1)
  rows = torch.arange(th.shape[0], device=th.device)
  return th[rows, best], best, (~in_coll).any(1)


def measure(pl, io, per_problem, reps=100, rounds=4):
  dtype = torch.float32 if io == 'f32' else torch.float64
  g = torch.Generator().manual_seed(16)
  ends = lambda: torch.cat((torch.rand(B, 1, 2, generator=g, dtype=torch.float64) * 8 - 4, torch.zeros(B, 1, 2, dtype=torch.float64)), -1).to(dtype).to(dev)
  st, go = ends(), ends()
  with torch.no_grad():
    th = pl.sample_prior(st, go, S, seed=1, scale=0.3)[0]                                   # (B,S,n,4): smooth trajectories across the map
  score = torch.rand(B, S, generator=g, dtype=torch.float64).to(dtype).to(dev)
  exclude = torch.zeros(B, S, dtype=torch.int32, device=dev)
  one = torch.from_numpy(circles_sdf(G, CIRCLES)).to(dtype).to(dev).reshape(1, 1, G, G)
  sdf = one.expand(B, 1, G, G).contiguous() if per_problem else one
  layer = pl.plan_layer
  solver = layer._solver(dtype)
  stream = torch.cuda.current_stream().cuda_stream
  arg = solver.sdf_arg(sdf.data_ptr(), G, G, G * G if per_problem else 0)
  th_sm = th.transpose(0, 1).contiguous() if per_problem else None                          # what S solves of B rows leave behind
  src = th_sm if per_problem else th
  sc, ex = (score.T.contiguous(), exclude.T.contiguous()) if per_problem else (score, exclude)
  params = solver.select_params(K, 0.0, per_problem, True)
  th_best = torch.empty(B, N, 4, dtype=dtype, device=dev)
  best = torch.empty(B, dtype=torch.int32, device=dev)
  order, status = torch.empty(B, S, dtype=torch.int32, device=dev), torch.empty(B, S, dtype=torch.int32, device=dev)
  ssum, psum = torch.empty(B, S, 6, dtype=torch.float64, device=dev), torch.empty(B, 6, dtype=torch.float64, device=dev)
  launch = lambda: solver.select_samples(B, S, src.data_ptr(), params, sc.data_ptr(), ex.data_ptr(), arg, None, th_best.data_ptr(), best.data_ptr(), order.data_ptr(),
                                         status.data_ptr(), ssum.data_ptr(), psum.data_ptr(), stream)
  # the same launch without the gather (th_best NULL: no second barrier, no copy) and without sample_summary: what the epilogue behind the dense check costs
  lean = lambda: solver.select_samples(B, S, src.data_ptr(), params, sc.data_ptr(), ex.data_ptr(), arg, None, None, best.data_ptr(), None, status.data_ptr(), None, None, stream)
  # ... and the same B S trajectories as B S problems of ONE sample each (shared grid only): one wavefront per workgroup, the granularity of dgp_gp_interpolate,
  # with the limits / finiteness checks and the epilogue still in -- what the 8-wavefront workgroups cost
  flat_best, flat_status = torch.empty(B * S, dtype=torch.int32, device=dev), torch.empty(B * S, dtype=torch.int32, device=dev)
  p1 = solver.select_params(K, 0.0, False, True)
  single = None if per_problem else (lambda: solver.select_samples(B * S, 1, th.data_ptr(), p1, score.data_ptr(), exclude.data_ptr(), arg, None, None, flat_best.data_ptr(), None,
                                                                   flat_status.data_ptr(), None, None, stream))
  isum = torch.empty(B * S, 6, dtype=torch.float64, device=dev)
  if per_problem:
    def interp():
      for s in range(S): solver.gp_interpolate(B, th_sm[s].data_ptr(), K, arg, 0.0, None, None, isum[s * B:].data_ptr(), stream)
  else:
    interp = lambda: solver.gp_interpolate(B * S, th.data_ptr(), K, arg, 0.0, None, None, isum.data_ptr(), stream)
  launch(); interp(); torch.cuda.synchronize()
  agree = bool(torch.equal(ssum.view(B * S, 6), isum.view(S, B, 6).transpose(0, 1).reshape(B * S, 6) if per_problem else isum))
  in_coll = ssum[:, :, 0] != 0
  tsel = lambda: torch_selection(th, in_coll, score)
  ref_best = tsel()[1]
  same_choice = float((ref_best == best.long()).double().mean())                            # (the recipe ignores the limits: not expected to be 1)
  timer = _capi.KernelTimer(reps)
  bench.prewarm(lambda k: launch(), 0.3, 100)
  for _ in range(3): interp(); tsel()
  torch.cuda.synchronize()
  t_k, t_i, t_t, t_l, t_1 = [], [], [], [], []
  for _ in range(rounds):      # alternated: all three see the same clocks
    timer.reset()
    for _ in range(reps):
      timer.arm(); launch()
    torch.cuda.synchronize()
    t_k += [v * 1e3 for v in timer.durations_ms()]
    timer.reset()
    for _ in range(reps):
      timer.arm(); lean()
    torch.cuda.synchronize()
    t_l += [v * 1e3 for v in timer.durations_ms()]
    if single is not None:
      timer.reset()
      for _ in range(reps):
        timer.arm(); single()
      torch.cuda.synchronize()
      t_1 += [v * 1e3 for v in timer.durations_ms()]
    if per_problem: t_i += events_us(interp, 4, 5)
    else:
      timer.reset()
      for _ in range(reps):
        timer.arm(); interp()
      torch.cuda.synchronize()
      t_i += [v * 1e3 for v in timer.durations_ms()]
    t_t += events_us(tsel, 4, 5)
  sz = th.element_size()
  moved = B * S * N * 4 * sz + B * N * 4 * sz + B * S * (sz + 4) + B * S * (4 + 4 + 48) + B * (4 + 48)
  q, qi, qt = quartiles(t_k), quartiles(t_i), quartiles(t_t)
  floor_us = moved / (bench.HBM_PEAK_GBS * 1e3)
  shape = solver.select_launch_shape(S, K)
  return {'io': io, 'grids': 'per-problem' if per_problem else 'shared', 'launch_shape_lpt_waves_passes': list(shape), 'kernel_us': q, 'kernel_without_gather_and_sample_summary_us': quartiles(t_l),
          'kernel_one_sample_per_problem_one_wavefront_per_workgroup_us': quartiles(t_1) if t_1 else None,
          'interpolate_summary_only_us': qi, 'interpolate_launches': S if per_problem else 1, 'interpolate_timed_by': 'HIP events around the launches' if per_problem else 'dgp_time_next_launch',
          'torch_selection_ops_us': qt, 'replaced_total_us': round(qi['median'] + qt['median'], 2), 'replaced_over_kernel': round((qi['median'] + qt['median']) / q['median'], 2),
          'kernel_over_interpolate': round(q['median'] / qi['median'], 2), 'bytes_algorithmic': moved, 'hbm_floor_us': round(floor_us, 2),
          'hbm_roof_share': round(floor_us / q['median'], 4), 'sample_summary_equals_interpolate_bits': agree, 'share_of_problems_with_the_recipes_choice': round(same_choice, 4)}


def end_to_end(pl, io, reps=5):
  """plan_multistart against the old recipe on the shared grid, wall clock around a synchronisation (ms per call)"""
  dtype = torch.float32 if io == 'f32' else torch.float64
  g = torch.Generator().manual_seed(17)
  ends = lambda: torch.cat((torch.rand(B, 1, 2, generator=g, dtype=torch.float64) * 8 - 4, torch.zeros(B, 1, 2, dtype=torch.float64)), -1).to(dtype).to(dev)
  st, go = ends(), ends()
  one = torch.from_numpy(circles_sdf(G, CIRCLES)).to(dtype).to(dev).reshape(1, 1, G, G)
  shared = one.expand(B * S, 1, G, G)
  im = (one > 0).to(dtype).expand(B * S, 1, G, G)

  def new():
    return pl.plan_multistart(st, go, one, S, seed=2, scale=0.5, num_inter=K)[0]

  def old():
    th0 = pl.sample_prior(st, go, S, seed=2, scale=0.5)[0].flatten(0, 1)
    pl.lazy_results = True
    try: out = pl.forward(th0, st.repeat_interleave(S, 0), go.repeat_interleave(S, 0), im, shared)
    except RuntimeError as e: return 'forward() raised: %s' % str(e)[:120]      # one non-SPD sample aborts the batch
    err = torch.as_tensor(np.asarray(out[3]), device=dev).view(B, S)
    coll = pl.interpolate(out[0], K, shared, eps=0.0).in_collision.view(B, S)
    return torch_selection(out[0].view(B, S, N, 4), coll, err)[0]
  res = {}
  with torch.no_grad():
    for name, fn in (('plan_multistart_ms', new), ('old_recipe_ms', old)):
      r = fn(); torch.cuda.synchronize()
      if isinstance(r, str): res[name] = r; continue
      t = []
      for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
      res[name] = quartiles(t)
  return dict(io=io, **res)


def main():
  pl = planner()
  cases = [measure(pl, io, per) for io in ('f32', 'f64') for per in (False, True)]
  e2e = [end_to_end(pl, io) for io in ('f32', 'f64')]
  out = {'what': 'dgp_select_samples, B = %d problems, S = %d samples, n = %d, K = %d, %d x %d grids; kernel time by dgp_time_next_launch over back-to-back warmed launches, '
                 'alternated with what it replaces' % (B, S, N, K, G, G),
         'hbm_peak_GBps': bench.HBM_PEAK_GBS, 'device': torch.cuda.get_device_name(0), 'cases': cases, 'end_to_end_shared_grid': e2e,
         'not_measured': ['no hardware counters were collected: the share of the roof is bytes from the shapes over kernel time',
                          'the workgroup size (up to 16 wavefronts) and the LDS key layout were not varied',
                          'the old recipe on per-problem grids needs an S-fold copy of the grids (8 GiB in fp32 at this shape) and was not run end to end']}
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r16_select_samples.json')
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, 'w') as f: json.dump(out, f, indent=1)
  print(json.dumps(out, indent=1))


if __name__ == '__main__':
  main()
