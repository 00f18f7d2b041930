"""What the SDF lookup costs on the device, at B = 4096 rows of S = 64 points on 256 x 256 grids -- shared and per-sample, fp32 and fp64 -- written to
profiles/r12_sdf_lookup.json:

  1. kernel times of dgp_sdf_lookup (d_obs + J + summary) and dgp_sdf_lookup_backward (g_points + the dense grid gradient; the zero fill of that gradient is the
     caller's and is not in the kernel time) through dgp_time_next_launch (_capi.KernelTimer: warmed, repeated launches; median and quartiles), for the positions
     of a (B, n, 4) trajectory tensor read in place (point_stride 4) and for a dense (B, S, 2) array (point_stride 2: vector rows);
  2. next to each, the bytes the call must move -- points in + outputs (+ cotangents in) + the DISTINCT 128-byte lines its taps touch in the grids (backward: once
     more, twice, for the read-modify-write of the gradient cells) -- and the share of the HBM roof that gives;
  3. the comparison: utils.sdf_utils.bilinear_interpolate_torch -- the torch mirror, NOT the code under test -- as batched device ops on the same inputs, forward
     and forward + backward, by a host clock around synchronised repetitions.

usage: python profiles/tools/sdf_lookup_time.py [output.json]"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, S, G = 4096, 64, 256
X_LIMS, Y_LIMS = (-5.0, 5.0), (-5.0, 5.0)
RES = (X_LIMS[1] - X_LIMS[0]) / G
LINE = 128


def quartiles(t):
  t = np.asarray(t, np.float64)
  return {'median': round(float(np.median(t)), 2), 'q1': round(float(np.percentile(t, 25)), 2), 'q3': round(float(np.percentile(t, 75)), 2), 'min': round(float(t.min()), 2)}


def distinct_tap_lines(pts, H, W, esize, shared):
  """number of distinct 128-byte lines the four taps of every point touch in row-major grids of H x W elements of `esize` bytes (pts: (B, S, 2) numpy, float64)"""
  px = (0. - X_LIMS[0] / RES) + pts[:, :, 0] / RES
  py = (0. - Y_LIMS[0] / RES) - pts[:, :, 1] / RES
  x1 = np.floor(px).astype(np.int64); y1 = np.floor(py).astype(np.int64)
  x2, y2 = np.clip(x1 + 1, 0, W - 1), np.clip(y1 + 1, 0, H - 1)
  x1, y1 = np.clip(x1, 0, W - 1), np.clip(y1, 0, H - 1)
  base = (0 if shared else np.arange(pts.shape[0], dtype=np.int64)[:, None] * (H * W))
  lines = [((base + y * W + x) * esize) // LINE for y in (y1, y2) for x in (x1, x2)]
  return int(np.unique(np.concatenate([l.reshape(-1) for l in lines])).size)


def algorithmic_bytes(pts, esize, shared, stride):
  """(forward, backward) bytes: points in (whole rows of `stride` elements are fetched line by line: the two used elements are counted) + outputs + distinct tap lines"""
  n = pts.shape[0] * pts.shape[1]
  lines = distinct_tap_lines(pts, G, G, esize, shared) * LINE
  fwd = n * 2 * esize + n * 3 * esize + pts.shape[0] * 5 * 8 + lines
  bwd = n * 2 * esize + n * 3 * esize + n * 2 * esize + lines + 2 * lines
  return fwd, bwd, lines


if __name__ == '__main__':
  import torch
  import bench
  from dgpmp2_amd import _capi
  from dgpmp2_amd.utils import sdf_utils as SU
  dev = torch.device('cuda:0')
  assert torch.cuda.is_available(), 'sdf_lookup_time.py measures on the GPU'

  def measure(io, shared, reps=200, rounds=4):
    dtype = torch.float32 if io == 'f32' else torch.float64
    th, _, _, sdf = bench.make_inputs(B, S, G, dev)
    th = th.to(dtype).contiguous()                                     # (B, S, 4): straight-line trajectories, positions in columns 0, 1
    gen = torch.Generator().manual_seed(3)
    th[:, :, :2] += (0.2 * torch.randn((B, S, 2), generator=gen, dtype=torch.float64)).to(dtype).to(dev)
    dense = th[:, :, :2].contiguous()
    grid = sdf.to(dtype).reshape(1, G, G)
    if not shared: grid = (grid + 0.001 * torch.arange(B, device=dev, dtype=dtype)[:, None, None]).contiguous()
    g_d = torch.randn((B, S), generator=gen, dtype=torch.float64).to(dtype).to(dev)
    g_J = torch.randn((B, S, 2), generator=gen, dtype=torch.float64).to(dtype).to(dev)
    d, J, g_p = torch.empty((B, S), dtype=dtype, device=dev), torch.empty((B, S, 2), dtype=dtype, device=dev), torch.empty((B, S, 2), dtype=dtype, device=dev)
    summ = torch.empty((B, _capi.DGP_LOOKUP_COUNT), dtype=torch.float64, device=dev)
    g_s = torch.zeros_like(grid)
    pc, st, code = _capi.get_pycall(), torch.cuda.current_stream().cuda_stream, _capi.DGP_F32 if io == 'f32' else _capi.DGP_F64
    sd = (grid.data_ptr(), G, G, 0 if shared else G * G, _capi.DGP_SDF_ROWMAJOR, _capi.DGP_GSDF_DENSE, None)
    frame = (RES, X_LIMS[0], X_LIMS[1], Y_LIMS[0], Y_LIMS[1])
    out = {'io': io, 'grid': 'shared' if shared else 'per-sample'}
    esize = th.element_size()
    for name, pts, stride in (('trajectory_in_place_stride4', th, 4), ('dense_points_stride2', dense, 2)):
      fwd = lambda: pc.sdf_lookup(code, B, S, pts.data_ptr(), stride, *sd, *frame, 0.4, d.data_ptr(), J.data_ptr(), summ.data_ptr(), st)
      bwd = lambda: pc.sdf_lookup_backward(code, B, S, pts.data_ptr(), stride, *sd, *frame, g_d.data_ptr(), g_J.data_ptr(), g_p.data_ptr(), g_s.data_ptr(),
                                           0 if shared else G * G, 1, st)
      assert fwd() == 0 and bwd() == 0
      torch.cuda.synchronize()
      timer = _capi.KernelTimer(reps)
      bench.prewarm(lambda k: fwd(), 0.3, 100)
      acc = {'forward': [], 'backward': []}
      for _ in range(rounds):
        for launch, key in ((fwd, 'forward'), (bwd, 'backward')):
          timer.reset()
          for _ in range(reps):
            timer.arm(); launch()
          torch.cuda.synchronize()
          acc[key] += [v * 1e3 for v in timer.durations_ms()]
      fb, bb, lines = algorithmic_bytes(pts[:, :, :2].double().cpu().numpy(), esize, shared, stride)
      out[name] = {'distinct_tap_line_bytes': lines}
      for key, nbytes in (('forward', fb), ('backward', bb)):
        q = quartiles(acc[key])
        out[name][key] = {'kernel_us': q, 'launches': len(acc[key]), 'algorithmic_bytes': nbytes, 'effective_GBps': round(nbytes / q['median'] * 1e-3, 1),
                          'hbm_roof_share': round(nbytes / q['median'] * 1e-3 / bench.HBM_PEAK_GBS, 4)}
    # the torch mirror as batched device ops, on the dense points (its best case: no strided gather)
    want_d, want_J = SU.bilinear_interpolate_torch(grid.expand(B, G, G) if shared else grid, dense, RES, X_LIMS, Y_LIMS)
    torch.cuda.synchronize()
    # (d, J: the last forward launch ran on `dense`.  On the device torch divides by a host scalar through its reciprocal, so the mirror's px, py and J are not the
    #  kernel's bits there -- on the CPU they are, tests/test_hip_lookup.py -- and a point that lands on the other side of a cell line differs visibly in J)
    out['kernel_against_device_mirror'] = {'d_obs_max_abs_difference': float((want_d[:, :, 0].double() - d.double()).abs().max()),
                                           'J_median_abs_difference': float((want_J.double() - J.double()).abs().median()),
                                           'points_with_identical_bits': float(((want_d[:, :, 0] == d) & (want_J == J).all(-1)).double().mean())}
    mreps = 20 if shared else 5

    def mirror_fwd():
      with torch.no_grad(): SU.bilinear_interpolate_torch(grid.expand(B, G, G) if shared else grid, dense, RES, X_LIMS, Y_LIMS)

    def mirror_fwd_bwd():
      im, stt = grid.detach().requires_grad_(True), dense.detach().requires_grad_(True)
      dd, JJ = SU.bilinear_interpolate_torch(im.expand(B, G, G) if shared else im, stt, RES, X_LIMS, Y_LIMS)
      torch.autograd.grad((dd[:, :, 0] * g_d).sum() + (JJ * g_J).sum(), (im, stt))
    for key, f in (('mirror_forward_us', mirror_fwd), ('mirror_forward_backward_us', mirror_fwd_bwd)):
      for _ in range(3): f()
      torch.cuda.synchronize()
      ts = []
      for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(mreps): f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / mreps * 1e6)
      out[key] = quartiles(ts)
    k = out['dense_points_stride2']
    out['mirror_forward_over_kernel'] = round(out['mirror_forward_us']['median'] / k['forward']['kernel_us']['median'], 1)
    out['mirror_forward_backward_over_kernels'] = round(out['mirror_forward_backward_us']['median'] / (k['forward']['kernel_us']['median'] + k['backward']['kernel_us']['median']), 1)
    return out

  res = {'config': 'B=%d rows of S=%d points, %dx%d grids, res %g, straight-line trajectories with 0.2 noise' % (B, S, G, G, RES), 'hbm_peak_GBps': bench.HBM_PEAK_GBS,
         'method': {'kernel_us': 'dgp_time_next_launch events per launch (200 launches x 4 rounds per variant, after a 0.3 s pre-warm); the forward writes d_obs, J and the summary, '
                                 'the backward g_points and the dense grid gradient (dtype accumulators; zero fill by the caller, not timed)',
                    'algorithmic_bytes': 'points in (two elements per point) + outputs (+ cotangents) + distinct 128-byte tap lines of the grids; backward: the tap lines once for the '
                                         'grid and twice for the read-modify-write of the gradient',
                    'mirror': 'utils.sdf_utils.bilinear_interpolate_torch as batched torch ops on the same device tensors; host clock around synchronised repetitions (includes '
                              'launch gaps: it is a call time, the kernel figures are kernel times)'},
         'cases': [measure(io, shared) for io in ('f32', 'f64') for shared in (True, False)]}
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r12_sdf_lookup.json')
  with open(path, 'w') as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res))
