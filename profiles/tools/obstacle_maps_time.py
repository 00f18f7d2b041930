"""Kernel time of dgp_obstacle_maps (dgp_time_next_launch events, _capi.KernelTimer, back-to-back launches; median and minimum) at E = 4096 maps of 256 x 256,
`forest` and `passage` with the reference's separations (generate_2d_dataset.py:196-208 for the example robot), uint8 and float64 images, next to
  * a plain device fill of the same output tensor (torch's fill kernel, HIP events around it): the floor of the painting phase -- the same bytes stored once;
  * a reference-style host generator on a few maps: one Python rejection loop per obstacle that copies and repaints the whole NumPy map for every candidate, the
    way obst_generator.py does it (wall clock per map; np.random in place of random.randint; at most 100 candidates per obstacle, where the reference has no bound
    and never returns once two obstacles overlap).
Prints one JSON line.   usage: python profiles/tools/obstacle_maps_time.py"""
import json, math, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench
from dgpmp2_amd import _capi
from dgpmp2_amd.datasets.obstacle_maps import dataset_params, reference_separations
from dgpmp2_amd.gpmp2.plan_layer import solver_config

dev = torch.device('cuda:0')
E, S = 4096, 256
s = _capi.Solver(solver_config(num_states=64, dof=2, io_dtype=torch.float64))
st = torch.cuda.current_stream().cuda_stream
KINDS = {'rect': _capi.DGP_OBST_RECT, 'wall': _capi.DGP_OBST_WALL}
CODES = {torch.uint8: _capi.DGP_U8, torch.float64: _capi.DGP_F64}


def params_of(dataset_type):
  sgd, sep = reference_separations(dataset_type, 0.4, 0.4, (-5.0, 5.0), S)
  p = dataset_params(dataset_type, S, sgd, sep)
  return p, s.obstacle_params(KINDS[p['kind']], **{k: v for k, v in p.items() if k != 'kind'})


def kernel_us(launch, reps=60):
  timer = _capi.KernelTimer(reps)
  bench.prewarm(lambda k: launch(), 0.3, 20)
  for _ in range(reps):
    timer.arm(); launch()
  torch.cuda.synchronize()
  t = np.asarray(timer.durations_ms()) * 1e3
  return float(np.median(t)), float(t.min())


def events_us(fn, reps=60):
  bench.prewarm(lambda k: fn(), 0.3, 20)
  ts = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    ts.append(a.elapsed_time(b) * 1e3)
  return float(np.median(ts)), float(np.min(ts))


def host_map(p, rs, max_draws=100):      # (the reference has no bound: once two obstacles overlap it never returns)
  """one map the reference's way (rectangles / walls, no keep-out points): copy, paint, test, per candidate"""
  m = np.zeros((S, S))
  half = lambda v: int(math.ceil(v / 2))
  pad = half(p['patch_size_obs'])
  for _ in range(rs.randint(p['n_lo'], p['n_hi'])):
    for k in range(max_draws):
      w, h = rs.randint(p['w_min'], p['w_max'] + 1), rs.randint(p['h_min'], p['h_max'] + 1)
      if p['kind'] == 'wall':
        cx, gy = rs.randint(p['start_x'] + half(w), S - half(w) + 1), rs.randint(p['start_y'] + half(h), S - half(h) + 1)
        body = [(slice(0, gy - half(h)), slice(cx - half(w), cx + half(w))), (slice(gy + half(h), None), slice(cx - half(w), cx + half(w)))]
        grown = body
      else:
        cx, cy = rs.randint(p['start_x'] + half(w), p['end_x'] - half(w) + 1), rs.randint(p['start_y'] + half(h), p['end_y'] - half(h) + 1)
        body = [(slice(cy - half(h), cy + half(h)), slice(cx - half(w), cx + half(w)))]
        grown = [(slice(cy - half(h) - pad, cy + half(h) + pad), slice(cx - half(w) - pad, cx + half(w) + pad))]
      t = np.copy(m)
      for r, c in grown: t[r, c] += 1
      if not np.any(t > 1): break
    for r, c in body: m[r, c] += 1
  return 1 - m


out = {'config': 'E=%d maps of %dx%d, reference separations of the example robot' % (E, S, S)}
for dataset_type in ('forest', 'passage'):
  pd, pc = params_of(dataset_type)
  for dtype in (torch.uint8, torch.float64):
    image = torch.empty((E, S, S), dtype=dtype, device=dev)
    boxes, draws = torch.empty((E, 64, 4), dtype=torch.int32, device=dev), torch.empty((E, 64), dtype=torch.int32, device=dev)
    num_boxes, info = torch.empty((E,), dtype=torch.int32, device=dev), torch.empty((E,), dtype=torch.int32, device=dev)

    def launch(): s.obstacle_maps(E, S, S, pc, image.data_ptr(), CODES[dtype], seed=1, boxes=boxes.data_ptr(), num_boxes=num_boxes.data_ptr(), draws=draws.data_ptr(),
                                  info=info.data_ptr(), stream=st)
    launch(); torch.cuda.synchronize()
    fl, dr = info.cpu().numpy(), draws.cpu().numpy()
    med, mn = kernel_us(launch)
    f_med, f_mn = events_us(lambda: image.fill_(1))
    key = '%s_%s' % (dataset_type, 'u8' if dtype is torch.uint8 else 'f64')
    out[key] = {'kernel_us': round(med, 1), 'kernel_us_min': round(mn, 1), 'fill_us': round(f_med, 1), 'fill_us_min': round(f_mn, 1), 'image_MiB': image.numel() * image.element_size() >> 20,
                'kernel_GB_per_s': round(image.numel() * image.element_size() / med / 1e3, 0), 'mean_obstacles': round(float((dr >= 0).sum(1).mean()), 1),
                'mean_draws_per_obstacle': round(float((dr[dr >= 0] + 1).mean()), 2), 'capped': int((fl & 1 != 0).sum()), 'overlapping': int((fl & 2 != 0).sum()),
                'wrapped': int((fl & 4 != 0).sum())}
    del image
  rs = np.random.RandomState(0)
  t0 = time.perf_counter()
  n_host = 4
  for _ in range(n_host): host_map(pd, rs)
  out[dataset_type + '_host_ms_per_map'] = round((time.perf_counter() - t0) / n_host * 1e3, 2)
  out[dataset_type + '_host_s_for_batch'] = round((time.perf_counter() - t0) / n_host * E, 1)
print(json.dumps(out))
