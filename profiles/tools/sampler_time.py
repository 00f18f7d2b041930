"""Kernel time of dgp_sample_problems (dgp_time_next_launch events, _capi.KernelTimer, back-to-back launches) at B = 4096, n = 64 on the benchmark's shared 256 x 256
grid, fp32 I/O, next to
  * a batched-torch restatement of ONE rejection round on the same device (one start and one goal candidate per problem from torch.rand, the bilinear lookup, the two
    feasibility masks, the distance test and the straight-line trajectory as whole-batch torch ops; HIP events around the op sequence) -- a torch sampler needs
    several such rounds plus a host decision after each;
  * the reference-style host loop on a subset: a Python rejection loop per problem that tests one point per iteration with a dozen small torch ops on host tensors,
    the way get_random_2d_confs calls Env2D.is_feasible (wall clock per problem).
Prints one JSON line.   usage: python profiles/tools/sampler_time.py"""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2.plan_layer import solver_config

dev = torch.device('cuda:0')
B, n, G = 4096, 64, 256
CLEAR, MARGIN, T_SEC = 0.9, 0.5, 10.0
_, _, _, sdf = bench.make_inputs(B, n, G, dev)
sdf = sdf.float().contiguous()
s = _capi.Solver(solver_config(num_states=n, dof=2, io_dtype=torch.float32))
arg = s.sdf_arg(sdf.data_ptr(), G, G, 0)
sp = s.sample_params(CLEAR)
start, goal = torch.empty(B, 1, 4, device=dev), torch.empty(B, 1, 4, device=dev)
th = torch.empty(B, n, 4, device=dev)
draws, info = torch.empty(B, 2, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
st = torch.cuda.current_stream().cuda_stream


def sample(): s.sample_problems(B, arg, sp, start.data_ptr(), goal.data_ptr(), th.data_ptr(), seed=1, draws=draws.data_ptr(), info=info.data_ptr(), stream=st)


def lookup(g, x, y, res):
  px, py = 5.0 / res + x / res, 5.0 / res - y / res
  x1, y1 = torch.floor(px).long(), torch.floor(py).long()
  x2, y2 = (x1 + 1).clamp(0, G - 1), (y1 + 1).clamp(0, G - 1)
  x1, y1 = x1.clamp(0, G - 1), y1.clamp(0, G - 1)
  return (x2 - px) * (y2 - py) * g[y1, x1] + (px - x1) * (y2 - py) * g[y1, x2] + (x2 - px) * (py - y1) * g[y2, x1] + (px - x1) * (py - y1) * g[y2, x2]


g64 = sdf.double().reshape(G, G)
steps = torch.arange(n, device=dev, dtype=torch.float64).view(1, n, 1)


def torch_round():
  """one rejection round for the whole batch: candidates, feasibility, distance rule, initial trajectory"""
  lo, w = -5.0 + MARGIN, 10.0 - 2 * MARGIN
  c = lo + torch.rand(B, 4, device=dev, dtype=torch.float64) * w
  fs = lookup(g64, c[:, 0], c[:, 1], 10.0 / G) > CLEAR
  fg = lookup(g64, c[:, 2], c[:, 3], 10.0 / G) > CLEAR
  far = (c[:, 2:] - c[:, :2]).norm(dim=1) >= 0.6 * w * 2 ** 0.5
  ok = fs & fg & far
  sxy, gxy = c[:, None, :2], c[:, None, 2:]
  pos = sxy * (n - 1 - steps) / (n - 1) + gxy * steps / (n - 1)
  th0 = torch.cat([pos, ((gxy - sxy) / T_SEC).expand(B, n, 2)], -1).float()
  return ok, th0


g_host = g64.cpu()


def host_feasible(x, y):
  """one point, small torch ops on host tensors (the granularity of Env2D.is_feasible)"""
  p = torch.tensor([[x, y]], dtype=torch.float64)
  d = lookup(g_host, p[:, 0], p[:, 1], 10.0 / G)
  inlim = (p[:, 0] <= 5.0) & (p[:, 0] >= -5.0) & (p[:, 1] <= 5.0) & (p[:, 1] >= -5.0)
  d = torch.where(inlim, d, torch.tensor(10.0, dtype=torch.float64))
  return (d > CLEAR).item()


def host_loop(problems):
  rs = np.random.RandomState(0)
  lo, w = -5.0 + MARGIN, 10.0 - 2 * MARGIN
  t0 = time.perf_counter()
  for _ in range(problems):
    while True:
      sx, sy = lo + rs.rand() * w, lo + rs.rand() * w
      if host_feasible(sx, sy): break
    tries = 0
    while True:
      gx, gy = lo + rs.rand() * w, lo + rs.rand() * w
      if host_feasible(gx, gy):
        if ((gx - sx) ** 2 + (gy - sy) ** 2) ** 0.5 >= 0.6 * w * 2 ** 0.5 or tries > 15: break
        tries += 1
  return (time.perf_counter() - t0) / problems * 1e6


def kernel_us(launch, reps=400):
  timer = _capi.KernelTimer(reps)
  bench.prewarm(lambda k: launch(), 0.3, 100)
  for _ in range(reps):
    timer.arm(); launch()
  torch.cuda.synchronize()
  t = np.asarray(timer.durations_ms()) * 1e3
  return float(np.median(t)), float(t.min())


def events_us(fn, reps=50):
  bench.prewarm(lambda k: fn(), 0.3, 10)
  ts = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    ts.append(a.elapsed_time(b) * 1e3)
  return float(np.median(ts))


sample(); torch.cuda.synchronize()
dr, fl = draws.cpu().numpy(), info.cpu().numpy()
med, mn = kernel_us(sample)
ok, _ = torch_round()
host_us = host_loop(64)
print(json.dumps({'config': 'B=%d n=%d shared %dx%d grid fp32 I/O clearance %.1f' % (B, n, G, G, CLEAR), 'sample_problems_kernel_us': round(med, 2),
                  'sample_problems_kernel_us_min': round(mn, 2), 'mean_draws_start_goal': [round(float(v), 2) for v in (dr.mean(0) + 1)], 'max_draws_start_goal': [int(v) for v in dr.max(0) + 1],
                  'info_nonzero': int((fl != 0).sum()), 'torch_one_round_us': round(events_us(torch_round), 1), 'torch_one_round_acceptance': round(float(ok.double().mean()), 3),
                  'host_loop_us_per_problem': round(host_us, 1), 'host_loop_problems': 64, 'host_loop_us_for_batch': round(host_us * B, 0)}))
