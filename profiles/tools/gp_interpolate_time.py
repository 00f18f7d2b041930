"""Kernel time of dgp_gp_interpolate (dgp_time_next_launch events, _capi.KernelTimer: warmed, repeated launches; median and quartiles) at B = 4096, n = 64,
K in {0, 7, 15}, shared 256 x 256 grid, fp32 and fp64 I/O -- with all three outputs and with the summary alone -- next to the bytes the call must move (from the
shapes), the share of the HBM roof that gives, and the torch restatement of the same work on the same device in the same process, alternated with the kernel:
utils.planner_utils.gp_interpolate_traj plus the bilinear lookup, hinge and summary as batched torch ops (HIP events around the op sequence).
Writes profiles/r10_gp_interpolate.json and prints it.
usage: python profiles/tools/gp_interpolate_time.py [output.json]"""
import json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2.plan_layer import solver_config
from dgpmp2_amd.utils.planner_utils import gp_interpolate_traj

dev = torch.device('cuda:0')
B, n, G, d = 4096, 64, 256, 4
LAUNCH_FLOOR_US = 3.0      # below this a kernel time says nothing about bandwidth: an empty kernel's begin-to-end on this device is of that order
th0, _, _, sdf0 = bench.make_inputs(B, n, G, dev)
th0 = th0 + 0.05 * torch.randn(th0.shape, generator=torch.Generator().manual_seed(1), dtype=th0.dtype).to(dev)
pc = _capi.get_pycall()
st = torch.cuda.current_stream().cuda_stream


def quartiles(t):
  t = np.asarray(t, np.float64)
  return {'median': round(float(np.median(t)), 2), 'q1': round(float(np.percentile(t, 25)), 2), 'q3': round(float(np.percentile(t, 75)), 2), 'min': round(float(t.min()), 2)}


def torch_restatement(th, sdf, K):
  """the same outputs with batched torch ops in fp64: dense trajectory, hinge cost of every dense state, the six summary columns"""
  x = gp_interpolate_traj(th.double(), 10.0, n - 1, K)
  g = sdf.double().reshape(G, G)
  res = 10.0 / G
  px, py = 5.0 / res + x[..., 0] / res, 5.0 / res - x[..., 1] / res
  x1, y1 = torch.floor(px).long(), torch.floor(py).long()
  x2, y2 = (x1 + 1).clamp(0, G - 1), (y1 + 1).clamp(0, G - 1)
  x1, y1 = x1.clamp(0, G - 1), y1.clamp(0, G - 1)
  dist = (x2 - px) * (y2 - py) * g[y1, x1] + (px - x1) * (y2 - py) * g[y1, x2] + (x2 - px) * (py - y1) * g[y2, x1] + (px - x1) * (py - y1) * g[y2, x2]
  cost = torch.where(dist <= 0.4, 0.4 - dist, torch.zeros_like(dist))
  inner = cost[:, 1:-1]
  hit = inner != 0
  cnt = hit.sum(1)
  mx, worst = inner.max(1)
  first = torch.where(cnt > 0, hit.to(torch.int8).argmax(1) + 1, torch.full_like(cnt, -1))
  return x, cost, torch.stack([(cnt > 0).double(), cnt.double(), inner.mean(1), mx, first.double(), (worst + 1).double()], 1)


def measure(io, K, reps=300, rounds=6):
  dtype = torch.float32 if io == 'f32' else torch.float64
  th, sdf = th0.to(dtype).contiguous(), sdf0.to(dtype).contiguous()
  s = _capi.Solver(solver_config(num_states=n, dof=2, io_dtype=dtype))
  nd = (n - 1) * (K + 1) + 1
  dense = torch.empty(B, nd, d, dtype=dtype, device=dev)
  cost = torch.empty(B, nd, dtype=dtype, device=dev)
  summ = torch.empty(B, _capi.DGP_DENSE_COUNT, dtype=torch.float64, device=dev)
  grid = (sdf.data_ptr(), G, G, 0, 0, 0, None)
  full = lambda: pc.gp_interpolate(s.h, B, th.data_ptr(), K, *grid, 0.0, dense.data_ptr(), cost.data_ptr(), summ.data_ptr(), st)
  only = lambda: pc.gp_interpolate(s.h, B, th.data_ptr(), K, *grid, 0.0, None, None, summ.data_ptr(), st)
  assert full() == 0
  torch.cuda.synchronize()
  rx, rc, rs = torch_restatement(th, sdf, K)
  agree = {'th_dense': float((dense.double() - rx).abs().max()), 'dense_cost': float((cost.double() - rc).abs().max()),
           'summary_exact_columns_equal': bool(torch.equal(summ[:, [0, 1, 4, 5]], rs[:, [0, 1, 4, 5]]))}
  t_full, t_only, t_torch = [], [], []
  timer = _capi.KernelTimer(reps)
  bench.prewarm(lambda k: full(), 0.3, 100)
  for _ in range(rounds):      # kernel and torch restatement alternated: both see the same clocks
    for launch, acc in ((full, t_full), (only, t_only)):
      timer.reset()
      for _ in range(reps):
        timer.arm(); launch()
      torch.cuda.synchronize()
      acc += [v * 1e3 for v in timer.durations_ms()]
    for _ in range(5):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record(); torch_restatement(th, sdf, K); b.record(); torch.cuda.synchronize()
      t_torch.append(a.elapsed_time(b) * 1e3)
  sz = th.element_size()
  moved_full = B * n * d * sz + G * G * sz + B * nd * d * sz + B * nd * sz + B * _capi.DGP_DENSE_COUNT * 8      # th in, the shared grid once, th_dense, dense_cost, summary out
  moved_only = B * n * d * sz + G * G * sz + B * _capi.DGP_DENSE_COUNT * 8
  qf, qo = quartiles(t_full), quartiles(t_only)
  roof = lambda moved, us: round(moved / us * 1e-3 / bench.HBM_PEAK_GBS, 4)
  bound = lambda moved, us: 'HBM bandwidth' if moved / us * 1e-3 > 0.5 * bench.HBM_PEAK_GBS else ('launch and one round of memory latency' if us < 2 * LAUNCH_FLOOR_US else 'neither the HBM roof nor the launch floor: address arithmetic, fp64 issue and lookup latency per dense state')
  return {'io': io, 'K': K, 'dense_states': nd, 'kernel_us_all_outputs': qf, 'kernel_us_summary_only': qo, 'bytes_moved_all_outputs': moved_full, 'bytes_moved_summary_only': moved_only,
          'hbm_roof_share_all_outputs': roof(moved_full, qf['median']), 'hbm_roof_share_summary_only': roof(moved_only, qo['median']),
          'effective_GBps_all_outputs': round(moved_full / qf['median'] * 1e-3, 1), 'bound_all_outputs': bound(moved_full, qf['median']), 'bound_summary_only': bound(moved_only, qo['median']),
          'torch_restatement_us': quartiles(t_torch), 'torch_over_kernel': round(float(np.median(t_torch)) / qf['median'], 1), 'max_abs_diff_to_torch_restatement': agree}


out = {'config': 'B=%d n=%d shared %dx%d grid, K in (0, 7, 15), fp32 and fp64 I/O' % (B, n, G, G), 'hbm_peak_GBps': bench.HBM_PEAK_GBS,
       'method': 'dgp_time_next_launch events per launch (300 launches x 6 rounds per variant, after a 0.3 s pre-warm); torch restatement: HIP events around the op sequence, 5 per round, alternated with the kernel',
       'rows': [measure(io, K) for io in ('f32', 'f64') for K in (0, 7, 15)]}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r10_gp_interpolate.json')
with open(path, 'w') as f:
  json.dump(out, f, indent=1)
print(json.dumps(out))
