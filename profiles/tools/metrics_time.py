"""Kernel time of dgp_traj_metrics (dgp_time_next_launch events, _capi.KernelTimer) at B = 4096, n = 64, shared 256 x 256 grid, fp32 I/O, next to dgp_eval_errors
(which reads the same trajectories and grid) measured the same way in the same process, and to the torch-op restatement of the same metrics for the whole batch on
the same device (HIP events around the op sequence; no nonzero(), no per-trajectory Python loop -- the cheapest way to write them in torch).  Prints one JSON line.
usage: python profiles/tools/metrics_time.py"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2.plan_layer import solver_config

dev = torch.device('cuda:0')
B, n, G, d = 4096, 64, 256, 4
th, start, goal, sdf = bench.make_inputs(B, n, G, dev)
th = (th + 0.05 * torch.randn(th.shape, generator=torch.Generator().manual_seed(1), dtype=th.dtype).to(dev)).float().contiguous()
start, goal, sdf = start.float().contiguous(), goal.float().contiguous(), sdf.float().contiguous()
th_opt = (th + 0.1).contiguous()
s = _capi.Solver(solver_config(num_states=n, dof=2, io_dtype=torch.float32))
pc = _capi.get_pycall()
raw = torch.empty(B, _capi.DGP_METRIC_COUNT, dtype=torch.float64, device=dev)
oerr = torch.empty(B, n, device=dev)
outs = [torch.empty(B, device=dev) for _ in range(5)]
st = torch.cuda.current_stream().cuda_stream
grid = (sdf.data_ptr(), G, G, 0, 0, 0, None)


def metrics(): pc.traj_metrics(s.h, B, th.data_ptr(), *grid, 0.0, th_opt.data_ptr(), raw.data_ptr(), oerr.data_ptr(), st)
def metrics_only(): pc.traj_metrics(s.h, B, th.data_ptr(), *grid, 0.0, None, raw.data_ptr(), None, st)
def errors(): pc.eval_errors(s.h, B, th.data_ptr(), start.data_ptr(), goal.data_ptr(), *grid, 0, None, None, None, *[o.data_ptr() for o in outs], st)


def torch_metrics():
  """the same thirteen numbers per trajectory with batched torch ops (fp64, as the reference computes them)"""
  x, o, g = th.double(), th_opt.double(), sdf.double().reshape(G, G)
  res, steps, dt = 10.0 / G, n - 1.0, 10.0 / (n - 1.0)
  px, py = 5.0 / res + x[..., 0] / res, 5.0 / res - x[..., 1] / res
  x1, y1 = torch.floor(px).long(), torch.floor(py).long()
  x2, y2 = (x1 + 1).clamp(0, G - 1), (y1 + 1).clamp(0, G - 1)
  x1, y1 = x1.clamp(0, G - 1), y1.clamp(0, G - 1)
  dist = (x2 - px) * (y2 - py) * g[y1, x1] + (px - x1) * (y2 - py) * g[y1, x2] + (x2 - px) * (py - y1) * g[y2, x1] + (px - x1) * (py - y1) * g[y2, x2]
  err = torch.where(dist <= 0.4, 0.4 - dist, torch.zeros_like(dist))
  inner = err[:, 1:-1]
  cnt = (inner != 0).sum(1)
  d1 = x[:, 1:] - x[:, :-1]
  d2 = d1[:, 1:] - d1[:, :-1]
  e = torch.cat([x[:, 1:, :2] - (x[:, :-1, :2] + dt * x[:, :-1, 2:]), d1[..., 2:]], -1)
  sq = (x - o) ** 2
  return torch.stack([x[..., 2:].norm(dim=-1).mean(1), (d1[..., 2:] / steps).norm(dim=-1).mean(1), (d2[..., 2:] / steps ** 2).norm(dim=-1).mean(1), (e ** 2).mean((1, 2)),
                      (cnt > 0).double(), cnt.double(), inner.mean(1), inner.max(1).values, 1.5 * cnt * dt / 10.0, torch.zeros(B, device=dev, dtype=torch.float64),
                      sq[..., :2].mean((1, 2)), sq[..., 2:].mean((1, 2)), sq.mean((1, 2))], 1), err


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


metrics(); torch.cuda.synchronize()
ref, ref_err = torch_metrics()
agree = float(((raw - ref).abs().max(0).values / ref.abs().max(0).values.clamp_min(1e-300)).max())
m_med, m_min = kernel_us(metrics)
mo_med, _ = kernel_us(metrics_only)
e_med, e_min = kernel_us(errors)
sz = th.element_size()
moved = B * n * d * sz * 2 + G * G * sz + B * _capi.DGP_METRIC_COUNT * 8 + B * n * sz      # th, th_opt, the shared grid once, metrics out, obs_error out
print(json.dumps({'config': 'B=%d n=%d shared %dx%d grid fp32 I/O' % (B, n, G, G), 'traj_metrics_kernel_us': round(m_med, 2), 'traj_metrics_kernel_us_min': round(m_min, 2),
                  'traj_metrics_no_th_opt_no_obs_error_us': round(mo_med, 2), 'eval_errors_kernel_us': round(e_med, 2), 'eval_errors_kernel_us_min': round(e_min, 2),
                  'ratio_to_eval_errors': round(m_med / e_med, 2), 'bytes_moved': moved, 'effective_GBps': round(moved / m_med * 1e-3, 1),
                  'torch_ops_restatement_us': round(events_us(torch_metrics), 1), 'max_rel_diff_to_torch_restatement': agree}))
