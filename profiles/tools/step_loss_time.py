"""What the training loss costs on the device, at B = 4096, n = 64, dof 2, fp32 and fp64 I/O -- three measurements, written to profiles/r11_step_loss.json:

  1. kernel times through dgp_time_next_launch (_capi.KernelTimer: warmed, repeated launches; median and quartiles): the first forward launch of dgp_step_loss
     (loss_rows; the request goes to the first kernel an entry point launches) and the backward launch, next to the bytes each must move and the share of the HBM roof
     that gives.  The second forward launch (loss_batch, one workgroup) has no event pair of its own: its time comes from the kernel trace of measurement 3.
  2. the whole iteration -- forward_with_errors + loss + backward of `total` w.r.t. the trajectory and the three covariance tensors -- replayed through
     planner.graphed_iteration in the same process on the same inputs, once with utils.learn_utils.one_step_loss_torch (the torch formulation: what a training loop
     ran before dgp_step_loss existed, the baseline) and once with planner.step_loss; rounds of replays alternated, median and quartiles over the rounds.
  3. the kernels of one replayed iteration, for both, from a plain kernel trace taken in runs of their own:
         rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python profiles/tools/step_loss_time.py --replay torch|device N
     at two replay counts; `--count` turns the four traces into kernels per replay (the difference of the two counts over the difference of N) and the median
     duration of the three loss kernels.

usage: python profiles/tools/step_loss_time.py [--counts counts.json] [output.json]
       python profiles/tools/step_loss_time.py --replay torch|device N
       python profiles/tools/step_loss_time.py --count torch_lo.csv torch_hi.csv device_lo.csv device_hi.csv N_lo N_hi counts.json"""
import csv, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, n, G, d, DOF = 4096, 64, 256, 4, 2
WEIGHTS = dict(vel_loss_lambda=0.5, ext_obs_lambda=2.0, ext_loss_weight=0.3)
LOSS_KERNELS = ('loss_rows', 'loss_batch', 'loss_backward')


def quartiles(t):
  t = np.asarray(t, np.float64)
  return {'median': round(float(np.median(t)), 2), 'q1': round(float(np.percentile(t, 25)), 2), 'q3': round(float(np.percentile(t, 75)), 2), 'min': round(float(t.min()), 2)}


def count_traces(paths, n_lo, n_hi, out_path):
  def read(path):
    rows = list(csv.DictReader(open(path)))
    names = [r['Kernel_Name'] for r in rows]
    dur = {}
    for k in LOSS_KERNELS:
      v = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3 for r in rows if k in r['Kernel_Name']]
      if v: dur[k] = quartiles(v); dur[k]['launches'] = len(v)
    return names, dur
  out = {'method': 'rocprofv3 --kernel-trace (no counters), one run per variant and replay count; kernels per replay = (rows at %d replays - rows at %d replays) / %d' % (n_hi, n_lo, n_hi - n_lo)}
  for variant, lo, hi in (('torch_loss', paths[0], paths[1]), ('device_loss', paths[2], paths[3])):
    (nl, _), (nh, dur) = read(lo), read(hi)
    per = {}
    for name in set(nh):
      k = (nh.count(name) - nl.count(name)) / float(n_hi - n_lo)
      short = name.replace('(anonymous namespace)::', '').split('(')[0][:120]      # (truncated names may coincide: their counts add)
      if k: per[short] = per.get(short, 0.0) + k
    out[variant] = {'kernels_per_replayed_iteration': (len(nh) - len(nl)) / float(n_hi - n_lo), 'by_kernel': dict(sorted(per.items(), key=lambda kv: -kv[1])),
                    'loss_kernel_us': dur}
  with open(out_path, 'w') as f:
    json.dump(out, f, indent=1)
  print(json.dumps(out))


if len(sys.argv) > 1 and sys.argv[1] == '--count':
  count_traces(sys.argv[2:6], int(sys.argv[6]), int(sys.argv[7]), sys.argv[8])
  sys.exit(0)

import torch
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.utils.learn_utils import one_step_loss_torch

dev = torch.device('cuda:0')


def make_planner():
  from dgpmp2_amd.gpmp2 import DiffGPMP2Planner
  from dgpmp2_amd.robot_models import PointRobot2D
  t = lambda v: torch.tensor(v, dtype=torch.float64)
  gp = {'Q_c_inv': torch.eye(2, dtype=torch.float64), 'K_s': t(0.01), 'K_g': t(0.01)}
  ob = {'cost_sigma': t(0.01), 'epsilon_dist': t(0.4)}
  pp = {'dof': 2, 'state_dim': 4, 'total_time_sec': 10.0, 'total_time_step': n - 1}
  op = {'method': 'gauss_newton', 'reg': 0.1, 'max_iters': 10, 'tol_err': 1e-3, 'tol_delta': 1e-4}
  return DiffGPMP2Planner(gp, ob, pp, op, {'x_lims': [-5.0, 5.0], 'y_lims': [-5.0, 5.0]}, PointRobot2D(t(0.4), B, n, use_cuda=True), batch_size=B, use_cuda=True)


def iteration_inputs(dtype):
  th0, start, goal, sdf = bench.make_inputs(B, n, G, dev)
  th0, start, goal, sdf = (t.to(dtype).contiguous() for t in (th0, start, goal, sdf))
  gen = torch.Generator().manual_seed(2)
  th_opt = th0 + (0.3 * torch.randn(th0.shape, generator=gen, dtype=torch.float64)).to(dtype).to(dev)
  th = th0.clone().requires_grad_(True)
  qc = torch.eye(2, device=dev, dtype=dtype).expand(B, n - 1, 2, 2).contiguous().requires_grad_(True)
  ow = torch.full((B, n, 1, 1), 1e4, device=dev, dtype=dtype, requires_grad=True)
  ep = torch.full((B, n, 1, 1), 0.4, device=dev, dtype=dtype, requires_grad=True)
  return (th, qc, ow, ep, th_opt), (start, goal, sdf.expand(B, 1, G, G))


def iterations(planner, fixed):
  """the two iterations, as functions of (th, qc, ow, ep, th_opt) -> (total, the four gradients)"""
  start, goal, sdfb = fixed

  def with_torch_loss(th, qc, ow, ep, th_opt):
    dth, _, _, sg, gp_, ob = planner.plan_layer.forward_with_errors(th, start, goal, None, sdfb, qc, ow, ep)
    total = one_step_loss_torch(dth, th_opt - th, sg, gp_, ob, WEIGHTS)[0]
    return (total,) + torch.autograd.grad(total, (th, qc, ow, ep))

  def with_device_loss(th, qc, ow, ep, th_opt):
    dth, _, _, sg, gp_, ob = planner.plan_layer.forward_with_errors(th, start, goal, None, sdfb, qc, ow, ep)
    total = planner.step_loss(dth, th, th_opt, (sg, gp_, ob), WEIGHTS).total
    return (total,) + torch.autograd.grad(total, (th, qc, ow, ep))
  return {'torch': with_torch_loss, 'device': with_device_loss}


if len(sys.argv) > 1 and sys.argv[1] == '--replay':      # measurement 3: capture, N replays, nothing else
  variant, N = sys.argv[2], int(sys.argv[3])
  planner = make_planner()
  args, fixed = iteration_inputs(torch.float32)
  it = planner.graphed_iteration(iterations(planner, fixed)[variant])
  it(*args)
  for _ in range(N - 1): it.replay(*args)
  torch.cuda.synchronize()
  print('replayed %s %d times' % (variant, N))
  sys.exit(0)


def kernel_times(io, reps=300, rounds=4):
  dtype = torch.float32 if io == 'f32' else torch.float64
  gen = torch.Generator().manual_seed(1)
  upd, tgt, sub = (torch.randn((B, n, d), generator=gen, dtype=torch.float64).to(dtype).to(dev) for _ in range(3))
  sg, gp_, ob = (torch.rand((B,), generator=gen, dtype=torch.float64).to(dtype).to(dev) for _ in range(3))
  terms = torch.empty(_capi.DGP_LOSS_COUNT, dtype=torch.float64, device=dev)
  per = torch.empty(B, _capi.DGP_LOSS_PER_TRAJ, dtype=torch.float64, device=dev)
  g = torch.full((), 0.5, dtype=torch.float64, device=dev)
  gu, gt, gs = (torch.empty_like(upd) for _ in range(3))
  ge = [torch.empty(B, dtype=dtype, device=dev) for _ in range(3)]
  pc, st, code = _capi.get_pycall(), torch.cuda.current_stream().cuda_stream, _capi.DGP_F32 if io == 'f32' else _capi.DGP_F64
  w = (WEIGHTS['vel_loss_lambda'], WEIGHTS['ext_obs_lambda'], WEIGHTS['ext_loss_weight'])
  fwd = lambda: pc.step_loss(code, B, n, DOF, upd.data_ptr(), tgt.data_ptr(), sub.data_ptr(), sg.data_ptr(), gp_.data_ptr(), ob.data_ptr(), *w, terms.data_ptr(), per.data_ptr(), st)
  bwd_all = lambda: pc.step_loss_backward(code, B, n, DOF, upd.data_ptr(), tgt.data_ptr(), sub.data_ptr(), *w, g.data_ptr(), gu.data_ptr(), gt.data_ptr(), gs.data_ptr(),
                                          ge[0].data_ptr(), ge[1].data_ptr(), ge[2].data_ptr(), st)
  bwd_loop = lambda: pc.step_loss_backward(code, B, n, DOF, upd.data_ptr(), tgt.data_ptr(), sub.data_ptr(), *w, g.data_ptr(), gu.data_ptr(), None, gs.data_ptr(),
                                           ge[0].data_ptr(), ge[1].data_ptr(), ge[2].data_ptr(), st)
  assert fwd() == 0 and bwd_all() == 0
  torch.cuda.synchronize()
  ref = one_step_loss_torch(upd.double(), tgt.double(), sg.double(), gp_.double(), ob.double(), WEIGHTS, target_sub=sub.double())
  agree = max(abs(float(a) - float(b)) / max(abs(float(b)), 1e-300) for a, b in zip(terms.tolist(), ref))
  timer = _capi.KernelTimer(reps)
  bench.prewarm(lambda k: fwd(), 0.3, 100)
  acc = {'forward_rows': [], 'backward_all_outputs': [], 'backward_training_loop': []}
  for _ in range(rounds):
    for launch, key in ((fwd, 'forward_rows'), (bwd_all, 'backward_all_outputs'), (bwd_loop, 'backward_training_loop')):
      timer.reset()
      for _ in range(reps):
        timer.arm(); launch()
      torch.cuda.synchronize()
      acc[key] += [v * 1e3 for v in timer.durations_ms()]
  sz = upd.element_size()
  arr = B * n * d * sz
  moved = {'forward_rows': 3 * arr + 3 * B * sz + B * _capi.DGP_LOSS_PER_TRAJ * 8, 'backward_all_outputs': 6 * arr + 3 * B * sz + 8, 'backward_training_loop': 5 * arr + 3 * B * sz + 8}
  out = {'io': io, 'relative_difference_to_torch_mirror': agree}
  for key, v in acc.items():
    q = quartiles(v)
    out[key] = {'kernel_us': q, 'launches': len(v), 'bytes_moved': moved[key], 'effective_GBps': round(moved[key] / q['median'] * 1e-3, 1),
                'hbm_roof_share': round(moved[key] / q['median'] * 1e-3 / bench.HBM_PEAK_GBS, 4)}
  return out


def whole_iteration(io, reps=200, rounds=15):
  import time
  dtype = torch.float32 if io == 'f32' else torch.float64
  planner = make_planner()
  args, fixed = iteration_inputs(dtype)
  fns = iterations(planner, fixed)
  its = {k: planner.graphed_iteration(f) for k, f in fns.items()}
  outs = {k: [t.clone() for t in it(*args)] for k, it in its.items()}
  torch.cuda.synchronize()
  rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))
  agree = {name: rel(a, b) for name, a, b in zip(('total', 'g_th', 'g_qc', 'g_ow', 'g_eps'), outs['device'], outs['torch'])}
  acc = {k: [] for k in its}
  for k in its:
    for _ in range(300): its[k].replay(*args)
  torch.cuda.synchronize()
  for _ in range(rounds):      # alternated: both see the same clocks
    for k, it in its.items():
      torch.cuda.synchronize(); t0 = time.perf_counter()
      for _ in range(reps): it.replay(*args)
      torch.cuda.synchronize()
      acc[k].append((time.perf_counter() - t0) / reps * 1e6)
  qt, qd = quartiles(acc['torch']), quartiles(acc['device'])
  spread = max(qt['q3'] - qt['q1'], qd['q3'] - qd['q1'])
  return {'io': io, 'replayed_iteration_us_torch_loss': qt, 'replayed_iteration_us_device_loss': qd, 'rounds': rounds, 'replays_per_round': reps,
          'device_minus_torch_us': round(qd['median'] - qt['median'], 2), 'quartile_spread_us': round(spread, 2),
          'device_loss_not_slower_than_torch_loss_beyond_the_spread': bool(qd['median'] <= qt['median'] + spread),
          'device_against_torch_max_relative_difference': agree}


counts, argv = None, sys.argv[1:]
if argv and argv[0] == '--counts':
  counts, argv = json.load(open(argv[1])), argv[2:]
out = {'config': 'B=%d n=%d dof %d, shared %dx%d grid, weights %s, fp32 and fp64 I/O' % (B, n, DOF, G, G, WEIGHTS), 'hbm_peak_GBps': bench.HBM_PEAK_GBS,
       'method': {'kernel_times': 'dgp_time_next_launch events per launch (300 launches x 4 rounds per variant, after a 0.3 s pre-warm); forward_rows is the first of the two forward '
                                  'launches, the second (loss_batch) is in kernel_trace; backward_training_loop: g_target NULL, as th_opt needs no gradient',
                  'whole_iteration': 'plan_layer.forward_with_errors + loss + autograd.grad(total, (th, qc_inv, obscov_inv, eps)) captured by planner.graphed_iteration, replayed without input '
                                     'copies; wall clock over 200 replays per round, 15 rounds per variant, alternated, same process, same inputs'},
       'kernel_times': [kernel_times(io) for io in ('f32', 'f64')], 'whole_iteration': [whole_iteration(io) for io in ('f32', 'f64')], 'kernel_trace': counts}
path = argv[0] if argv else os.path.join(ROOT, 'profiles', 'r11_step_loss.json')
with open(path, 'w') as f:
  json.dump(out, f, indent=1)
print(json.dumps(out))
