"""Kernel time of dgp_prior_samples (dgp_time_next_launch events, _capi.KernelTimer: warmed, repeated launches; median and quartiles) at B = 4096, S = 8, n = 64,
dof 2 and 3, fp32 and fp64 I/O, mean NULL and given, noise generated and supplied -- next to the bytes the call must move (from the shapes: th written, plus the
mean and the supplied noise read), the share of the HBM roof that gives, and the torch mirror of the same work on the same device in the same process, alternated
with the kernel: utils.planner_utils.gp_prior_samples_torch on the same normals (plus torch.randn of the same shape where the kernel generates them), as the time
per call of several back-to-back calls between two HIP events, after a warm-up of its own; a call includes the mirror's host set-up (the constants and W_k,
copied over).  Writes profiles/r14_prior_samples.json and prints it.
usage: python profiles/tools/prior_samples_time.py [output.json]"""
import json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2.plan_layer import solver_config
from dgpmp2_amd.utils.planner_utils import gp_prior_samples_torch

dev = torch.device('cuda:0')
B, S, n = 4096, 8, 64
MIRROR_CALLS = 4
pc = _capi.get_pycall()
st = torch.cuda.current_stream().cuda_stream


def quartiles(t):
  t = np.asarray(t, np.float64)
  return {'median': round(float(np.median(t)), 2), 'q1': round(float(np.percentile(t, 25)), 2), 'q3': round(float(np.percentile(t, 75)), 2), 'min': round(float(t.min()), 2)}


def measure(dof, io, with_mean, supplied, reps=100, rounds=4):
  dtype = torch.float32 if io == 'f32' else torch.float64
  d = 2 * dof
  g = torch.Generator().manual_seed(dof)
  start = torch.cat((torch.rand(B, 1, dof, generator=g, dtype=torch.float64) * 8 - 4, torch.zeros(B, 1, dof, dtype=torch.float64)), -1).to(dtype).to(dev)
  goal = torch.cat((torch.rand(B, 1, dof, generator=g, dtype=torch.float64) * 8 - 4, torch.zeros(B, 1, dof, dtype=torch.float64)), -1).to(dtype).to(dev)
  mean = (torch.rand(B, n, d, generator=g, dtype=torch.float64) * 6 - 3).to(dtype).to(dev) if with_mean else None
  s = _capi.Solver(solver_config(num_states=n, dof=dof, io_dtype=dtype))
  th = torch.empty(B, S, n, d, dtype=dtype, device=dev)
  noise = torch.empty(B, S, n + 1, d, dtype=torch.float64, device=dev)
  info = torch.empty(B, S, dtype=torch.int32, device=dev)
  mp = None if mean is None else mean.data_ptr()
  # the normals of seed 1, written once; the supplied-noise variant reads them back
  assert pc.prior_samples(s.h, B, S, start.data_ptr(), goal.data_ptr(), mp, 1.0, 1, 0, None, th.data_ptr(), noise.data_ptr(), info.data_ptr(), st) == 0
  torch.cuda.synchronize()
  ref = th.clone()
  launch = lambda: pc.prior_samples(s.h, B, S, start.data_ptr(), goal.data_ptr(), mp, 1.0, 1, 0, noise.data_ptr() if supplied else None, th.data_ptr(), None, info.data_ptr(), st)
  assert launch() == 0
  torch.cuda.synchronize()
  same = bool(torch.equal(th, ref))
  eye = [[1.0 if i == j else 0.0 for j in range(dof)] for i in range(dof)]

  def mirror():
    z = noise if supplied else torch.randn(B, S, n + 1, d, dtype=torch.float64, device=dev)
    return gp_prior_samples_torch(start.double(), goal.double(), z, 10.0, n - 1, eye, 0.01, 0.01, None if mean is None else mean.double(), 1.0).to(dtype)
  agree = float((gp_prior_samples_torch(start.double(), goal.double(), noise, 10.0, n - 1, eye, 0.01, 0.01, None if mean is None else mean.double(), 1.0) - ref.double()).abs().max())
  t_k, t_torch = [], []
  timer = _capi.KernelTimer(reps)
  bench.prewarm(lambda k: launch(), 0.3, 100)
  for _ in range(2): mirror()      # the mirror's own warm-up: first calls load code objects and pick algorithms
  torch.cuda.synchronize()
  for _ in range(rounds):      # kernel and torch mirror alternated: both see the same clocks
    timer.reset()
    for _ in range(reps):
      timer.arm(); launch()
    torch.cuda.synchronize()
    t_k += [v * 1e3 for v in timer.durations_ms()]
    for _ in range(3):      # MIRROR_CALLS back-to-back calls between two events: the host set-up of a call (below) runs while the device works on the call before
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      for _ in range(MIRROR_CALLS): mirror()
      b.record(); torch.cuda.synchronize()
      t_torch.append(a.elapsed_time(b) * 1e3 / MIRROR_CALLS)
  sz = th.element_size()
  written = B * S * n * d * sz + B * S * 4
  read = 2 * B * d * sz + (B * n * d * sz if with_mean else 0) + (B * S * (n + 1) * d * 8 if supplied else 0)
  q = quartiles(t_k)
  floor_us = (written + read) / (bench.HBM_PEAK_GBS * 1e3)
  return {'dof': dof, 'io': io, 'mean': 'given' if with_mean else 'NULL', 'noise': 'supplied' if supplied else 'generated', 'kernel_us': q, 'bytes_written': written, 'bytes_read': read,
          'hbm_floor_us': round(floor_us, 2), 'hbm_roof_share': round(floor_us / q['median'], 4), 'effective_GBps': round((written + read) / q['median'] * 1e-3, 1),
          'bound': 'HBM bandwidth' if floor_us / q['median'] > 0.5 else (
              'not the HBM roof; not profiled further -- no normals are drawn here: what is left is the 8-byte loads of a lane\'s noise row and the fp64 chain, S^-1 and W per state' if supplied
              else 'not the HBM roof: the normals (the difference to the supplied-noise row of the same shape) -- one Philox block and an fp64 log, sin, cos and sqrt per pair'),
          'torch_mirror_us': quartiles(t_torch), 'torch_over_kernel': round(float(np.median(t_torch)) / q['median'], 1), 'max_abs_diff_to_torch_mirror': agree,
          'supplied_noise_reproduces_generated_bits': same}


out = {'config': 'B=%d S=%d n=%d, K_s = K_g = 0.01, Q_c_inv = I, dof 2 and 3, fp32 and fp64 I/O, mean NULL / given, noise generated / supplied' % (B, S, n), 'hbm_peak_GBps': bench.HBM_PEAK_GBS,
       'method': 'dgp_time_next_launch events per launch (100 launches x 4 rounds per variant, after a 0.3 s pre-warm); torch mirror: per-call time over %d back-to-back calls between two HIP events after two warm-up calls, 3 such windows per round, alternated with the kernel; a call of the mirror also forms Q_c, S^-1 and W_k in float64 on the host and copies W_k (n d d doubles) to the device -- a call time, not a sum of kernel times' % MIRROR_CALLS,
       'rows': [measure(dof, io, m, sup) for dof in (2, 3) for io in ('f32', 'f64') for m in (False, True) for sup in (False, True)]}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r14_prior_samples.json')
with open(path, 'w') as f:
  json.dump(out, f, indent=1)
print(json.dumps(out))
