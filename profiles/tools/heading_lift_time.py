"""Kernel time of dgp_heading_lift (dgp_time_next_launch events, _capi.KernelTimer: warmed, back-to-back launches; median and quartiles) at B = 4096, n = 64, fp32 and
fp64 I/O: TANGENT / DIFF with generated turns and with supplied turns, LINEAR / KEEP -- next to the bytes the call must move (from the shapes: B n 10 elements, plus
start / goal, the end headings, the supplied turns and info), the share of the HBM roof that gives, and the torch mirror of the same work on the same device and
inputs in the same process, alternated with the kernel: utils.planner_utils.heading_lift_torch, as the time per call of several back-to-back calls between two HIP
events after a warm-up of its own.  The TANGENT / DIFF cases run at n = 640 as well (the block loop: two passes over ten blocks).  The `reading` of the file is
formed from the measured cases by reading() below, not written by hand.  Writes profiles/r15_heading_lift.json and prints it.
usage: python profiles/tools/heading_lift_time.py [output.json]"""
import json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.gpmp2.plan_layer import solver_config
from dgpmp2_amd.utils.planner_utils import heading_lift_torch

dev = torch.device('cuda:0')
B, N_SHORT, N_LONG = 4096, 64, 640      # n = 64: one block of 64 lanes per trajectory, one pass; n = 640: the block loop, two passes
MIRROR_CALLS = 4
CASES = (('tangent', 'diff', 'generated'), ('tangent', 'diff', 'supplied'), ('linear', 'keep', 'none'))
st = torch.cuda.current_stream().cuda_stream


def reading(cases):
  """What the numbers of THIS run say, per shape: the range of the roof share, what supplying the turns (no atan2) and what LINEAR / KEEP (no tangent, scan or atan2)
  change, and the conclusion those support -- none where they support none"""
  lines = []
  for n in sorted({c['n'] for c in cases}):
    here = [c for c in cases if c['n'] == n]
    share = [c['hbm_roof_share'] for c in here]
    text = 'n = %d: %.2f-%.2f of the HBM roof' % (n, min(share), max(share))
    worst = 0.0
    for io in sorted({c['io'] for c in here}):
      med = {(c['heading'], c['turns']): c['kernel_us']['median'] for c in here if c['io'] == io}
      gen = med.get(('tangent', 'generated'))
      if gen is None: continue
      for key, name in ((('tangent', 'supplied'), 'supplied turns'), (('linear', 'none'), 'LINEAR / KEEP')):
        if key in med:
          text += '; %s %s %+.2f us against generated turns (%.2f us)' % (io, name, med[key] - gen, gen)
          worst = max(worst, abs(med[key] - gen) / gen)
    if max(share) >= 0.5: text += ' -- at least half the roof: bound by its bytes'
    elif len(here) > 2 and worst <= 0.25: text += (' -- far below the roof, and neither atan2 nor the tangent work changes the time by more than %.0f %%: the latency of the passes over a '
                                                   'trajectory, not bandwidth or arithmetic' % (100 * worst))
    else: text += ' -- below the roof; these cases do not say what bounds it'
    lines.append(text)
  return lines


def quartiles(t):
  t = np.asarray(t, np.float64)
  return {'median': round(float(np.median(t)), 2), 'q1': round(float(np.percentile(t, 25)), 2), 'q3': round(float(np.percentile(t, 75)), 2), 'min': round(float(t.min()), 2)}


def paths(dtype, n):
  """B planar trajectories: arcs of seeded radius, centre and extent (every row has a tangent of its own), the constant velocities of path_to_traj_avg_vel"""
  g = torch.Generator().manual_seed(15)
  r = torch.rand(B, 1, generator=g, dtype=torch.float64) * 2 + 1
  a0 = torch.rand(B, 1, generator=g, dtype=torch.float64) * 6 - 3
  da = (torch.rand(B, 1, generator=g, dtype=torch.float64) * 2 + 0.5) * torch.where(torch.rand(B, 1, generator=g) < 0.5, -1.0, 1.0)
  a = a0 + da * torch.arange(n, dtype=torch.float64)[None] / (n - 1)
  p = torch.stack((r * torch.cos(a), r * torch.sin(a)), -1)
  v = ((p[:, -1] - p[:, 0]) / 10.0)[:, None].expand(B, n, 2)
  hs, hg = torch.rand(B, generator=g, dtype=torch.float64) * 6 - 3, torch.rand(B, generator=g, dtype=torch.float64) * 6 - 3
  return torch.cat((p, v), -1).to(dtype).to(dev), hs.to(dev), hg.to(dev)


def measure(io, heading, velocity, turns_mode, n=N_SHORT, reps=100, rounds=4):
  dtype = torch.float32 if io == 'f32' else torch.float64
  BLEND = (n - 1) // 4
  th2, hs, hg = paths(dtype, n)
  s = _capi.Solver(solver_config(num_states=n, dof=3, io_dtype=dtype))
  hp = _capi.Solver.heading_params(_capi.DGP_HEADING_TANGENT if heading == 'tangent' else _capi.DGP_HEADING_LINEAR, _capi.DGP_END_SUPPLIED, _capi.DGP_END_SUPPLIED,
                                   _capi.DGP_VEL_DIFF if velocity == 'diff' else _capi.DGP_VEL_KEEP, BLEND)
  start, goal = torch.empty(B, 1, 6, dtype=dtype, device=dev), torch.empty(B, 1, 6, dtype=dtype, device=dev)
  th = torch.empty(B, n, 6, dtype=dtype, device=dev)
  turns = torch.empty(B, n, dtype=torch.float64, device=dev)
  info = torch.empty(B, dtype=torch.int32, device=dev)
  # the turns of the path, written once; the supplied-turns variant reads them back
  s.heading_lift(B, hp, th2.data_ptr(), start.data_ptr(), goal.data_ptr(), th.data_ptr(), hs.data_ptr(), hg.data_ptr(), None, turns.data_ptr(), info.data_ptr(), st)
  torch.cuda.synchronize()
  tin = turns.data_ptr() if turns_mode == 'supplied' else None
  launch = lambda: s.heading_lift(B, hp, th2.data_ptr(), start.data_ptr(), goal.data_ptr(), th.data_ptr(), hs.data_ptr(), hg.data_ptr(), tin, None, info.data_ptr(), st)
  launch()
  torch.cuda.synchronize()
  mirror = lambda: heading_lift_torch(th2, 10.0, hs, hg, heading, 'supplied', velocity, BLEND, turns=turns if turns_mode == 'supplied' else None)
  agree = float((mirror()[2].double() - th.double()).abs().max())
  t_k, t_torch = [], []
  timer = _capi.KernelTimer(reps)
  bench.prewarm(lambda k: launch(), 0.3, 100)
  for _ in range(2): mirror()      # the mirror's own warm-up: first calls load code objects
  torch.cuda.synchronize()
  for _ in range(rounds):      # kernel and torch mirror alternated: both see the same clocks
    timer.reset()
    for _ in range(reps):
      timer.arm(); launch()
    torch.cuda.synchronize()
    t_k += [v * 1e3 for v in timer.durations_ms()]
    for _ in range(3):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      for _ in range(MIRROR_CALLS): mirror()
      b.record(); torch.cuda.synchronize()
      t_torch.append(a.elapsed_time(b) * 1e3 / MIRROR_CALLS)
  sz = th.element_size()
  moved = B * n * 10 * sz                                             # the algorithmic bytes: 4 columns read, 6 written
  extra = 2 * B * 6 * sz + 2 * B * 8 + B * 4 + (B * n * 8 if turns_mode == 'supplied' else 0)      # start / goal, the end headings, info, the supplied turns
  q = quartiles(t_k)
  floor_us = (moved + extra) / (bench.HBM_PEAK_GBS * 1e3)
  return {'n': n, 'blend': BLEND, 'io': io, 'heading': heading, 'velocity': velocity, 'turns': turns_mode, 'kernel_us': q, 'bytes_algorithmic': moved, 'bytes_optional_arrays': extra,
          'hbm_floor_us': round(floor_us, 2), 'hbm_roof_share': round(floor_us / q['median'], 4), 'effective_GBps': round((moved + extra) / q['median'] * 1e-3, 1),
          'torch_mirror_us_per_call': quartiles(t_torch), 'torch_over_kernel': round(float(np.median(t_torch)) / q['median'], 1), 'max_abs_diff_to_mirror': agree}


def main():
  cases = [measure(io, h, v, t) for io in ('f32', 'f64') for h, v, t in CASES]
  cases += [measure(io, h, v, t, N_LONG, reps=50, rounds=2) for io in ('f32', 'f64') for h, v, t in CASES[:2]]
  out = {'what': 'dgp_heading_lift, B = %d, n = %d and %d, blend = (n - 1) // 4, supplied end headings; kernel time by dgp_time_next_launch over back-to-back warmed launches'
                 % (B, N_SHORT, N_LONG),
         'hbm_peak_GBps': bench.HBM_PEAK_GBS, 'device': torch.cuda.get_device_name(0),
         'reading': reading(cases),
         'not_measured': ['the scan primitive (__shfl_up, the cross-lane network) was not compared against a DPP row-shift form',
                          'n = 640 is timed as it stands: no variant of the block loop (one pass, or the end constants formed per block) was timed against it',
                          'no hardware counters were collected: the share of the roof is bytes from the shapes over kernel time'],
         'cases': cases}
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r15_heading_lift.json')
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, 'w') as f: json.dump(out, f, indent=1)
  print(json.dumps(out, indent=1))


if __name__ == '__main__':
  main()
