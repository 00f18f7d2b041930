"""dgp_time_next_launch on every launch site of the library (csrc/dgp_launch.h), each at the smallest shape that reaches it: the unit launchers of the step kernels
(gn_device.h), the long-trajectory launcher (gn_long_inst.hip), an entry point of two launches (dgp_gn_step_errors, d = 6 with q_full tensors), dgp_traj_metrics,
dgp_sample_problems and dgp_obstacle_maps.

For each: the call once plain and once behind KernelTimer.arm() gives the same bits; after a synchronisation the armed call's events hold a positive, finite
duration; a further plain call succeeds, gives the same bits again and leaves that duration as it was -- the request was used up by the armed call, not left behind."""
import math

import numpy as np
import pytest
import torch

import harness
from dgpmp2_amd import _capi
from oracle import gpmp2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 3


def _problem(dof, n, G=16):
  """B straight-line trajectories inside the limits and one shared G x G grid, values exact in float32"""
  p = O.OracleParams(dof=dof, total_time_step=n - 1)
  rs = np.random.RandomState(11)
  f32 = lambda a: a.astype(np.float32).astype(np.float64)
  conf = lambda: np.concatenate([rs.uniform(-3, 3, (B, 1, 2)), rs.uniform(-1, 1, (B, 1, dof - 2))], -1)
  s, g = f32(conf()), f32(conf())
  th = f32(O.straight_line_trajb(s, g, p.total_time_sec, n - 1, dof))
  z = np.zeros((B, 1, dof))
  sdf = f32(O.circles_sdf(G, O.C2_CIRCLES)[None, None])
  return p, th, np.concatenate([s, z], -1), np.concatenate([g, z], -1), sdf


def _gn_step(n):
  p, th, start, goal, sdf = _problem(2, n)
  be = harness.Backend('hip')
  return lambda: be.step(p, th, start, goal, sdf, io='f32')


def _gn_step_errors_two_launches():
  p, th, start, goal, sdf = _problem(3, 8)
  qc = np.broadcast_to(4.0 * np.eye(6) + 0.5, (B, 7, 6, 6)).copy()      # Q^-1 itself (DGP_QC_QFULL): d = 6 general kernels, the error kernel behind the step
  be = harness.Backend('hip')
  return lambda: be.step_errors(p, th, start, goal, sdf, qc=qc, q_full=True, io='f32')


def _solver(n=8):
  return _capi.Solver(harness.config_from_oracle(O.OracleParams(dof=2, total_time_step=n - 1), 'f32'))


def _dev(a, dtype=torch.float32):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _host(*ts):
  torch.cuda.synchronize()
  return tuple(t.cpu().numpy() for t in ts)


def _traj_metrics():
  _, th, _, _, sdf = _problem(2, 8)
  s, th_d, sdf_d = _solver(), _dev(th), _dev(sdf)

  def call():
    metrics = torch.full((B, _capi.DGP_METRIC_COUNT), float('nan'), dtype=torch.float64, device=DEV)
    obs = torch.full((B, 8), float('nan'), dtype=torch.float32, device=DEV)
    s.traj_metrics(B, th_d.data_ptr(), s.sdf_arg(sdf_d.data_ptr(), 16, 16, 0), metrics=metrics.data_ptr(), obs_error=obs.data_ptr(), stream=_stream())
    return _host(metrics, obs)
  return call


def _sample_problems():
  s, sdf_d = _solver(), _dev(_problem(2, 8)[4])

  def call():
    start, goal = (torch.full((B, 1, 4), float('nan'), dtype=torch.float32, device=DEV) for _ in range(2))
    th = torch.full((B, 8, 4), float('nan'), dtype=torch.float32, device=DEV)
    draws, info = torch.full((B, 2), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    s.sample_problems(B, s.sdf_arg(sdf_d.data_ptr(), 16, 16, 0), s.sample_params(0.4, max_draws=64), start.data_ptr(), goal.data_ptr(), th.data_ptr(), seed=5,
                      draws=draws.data_ptr(), info=info.data_ptr(), stream=_stream())
    return _host(start, goal, th, draws, info)
  return call


def _obstacle_maps():
  s = _solver()
  gen = s.obstacle_params(_capi.DGP_OBST_RECT, 2, 5, 3, 8, 3, 8, start_x=0, start_y=0, end_x=32, end_y=32, max_draws=64)

  def call():
    image = torch.full((2, 32, 32), 7, dtype=torch.uint8, device=DEV)
    boxes = torch.full((2, 64, 4), -7, dtype=torch.int32, device=DEV)
    num_boxes = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    s.obstacle_maps(2, 32, 32, gen, image.data_ptr(), _capi.DGP_U8, seed=3, boxes=boxes.data_ptr(), num_boxes=num_boxes.data_ptr(), stream=_stream())
    return _host(image, boxes, num_boxes)
  return call


CASES = {
    'gn_step': lambda: _gn_step(8),
    'gn_step_long': lambda: _gn_step(257),
    'gn_step_errors_two_launches': _gn_step_errors_two_launches,
    'traj_metrics': _traj_metrics,
    'sample_problems': _sample_problems,
    'obstacle_maps': _obstacle_maps,
}


def _same_bits(a, b):
  return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('name', sorted(CASES))
def test_timed_launch_same_results_and_one_shot(name):
  call = CASES[name]()
  timer = _capi.KernelTimer(1)
  plain = call()
  for a in plain:
    if a.dtype.kind == 'f': assert np.isfinite(a).all(), '%s: an output was not written' % name
  timer.arm()
  timed = call()
  torch.cuda.synchronize()
  ms = timer.durations_ms()[0]
  print('%s: %.4f ms' % (name, ms))
  assert _same_bits(plain, timed), '%s: the timed launch computed something else' % name
  assert math.isfinite(ms) and ms > 0.0, (name, ms)
  again = call()
  torch.cuda.synchronize()
  assert _same_bits(plain, again), name
  assert timer.durations_ms()[0] == ms, '%s: the request outlived the call it was armed for' % name
